// qc_balance.hip - kernels and C ABI (include/qc_balance.h) of the MI355X-native
// batched balance controller.  gfx950 only; fails loudly without a HIP device.
//
// Replaces BalanceController::control()
//   quadruped_controller/src/quadruped_controller/balance_controller.cpp:98-330 (BC.cpp)
// for n independent robots per launch.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdio>
#include <cstring>
#include <new>
#include <string>
#include <utility>

#include "../../include/qc_balance.h"
#include "qc_device.hpp"
#include "qc_host.hpp"
#include "qc_plant.hpp"
#include "qc_plant_model.hpp"

namespace qc {

// ------------------------------------------------------------------ the kernel
// A group of G lanes = one robot (qc_device.hpp).  Primal active-set method on
// the per-foot cube states:
//   fresh robot  f^ = EQP(S0)  (S0 = no active face, or the warm-start word);
//                f = clamp(f^); if nothing was clamped f^ is feasible.
//   afterwards   f^ = EQP(S);  step f -> f^ until the first blocking face (add
//                it), or, after a full step, drop the face with the most
//                negative multiplier; stop when all multipliers are >= 0 (KKT).
// The QP is strictly convex (W > 0), so the KKT point is THE minimiser qpOASES
// returns in the reference (BC.cpp:177-210).
//
// A wavefront (one workgroup) fills once: its chunk of at most 64/G robots is
// assembled into the wave's input stock, every lane executes the same
// working-set recalculation in lockstep (straight-line, select-based code, no
// per-lane branches) until the wave's slowest robot has converged, the results
// go to the wave's output stock and a dense pass stores them.  Robots need
// between 1 and ~20 recalculations; the stragglers of one- and two-lane waves
// finish four lanes per robot (finish_on_four_lanes), and the hardware
// scheduler refills the chip with the next workgroup.
//
// LDS stock planes (see "Dense phases around the divergent solve" below).
// SP = plane stride in doubles = slots + 1 (odd), so that the lanes of one group (same
// slot, planes 3*FPL apart) fall into different banks; the dense side
// (plane[f][lane]) is conflict-free either way.  A wave only ever holds its 64/G robots, so its
// stock is 64/G slots - 9.2 KB instead of 18 KB at G = 2, which is what lets more than two workgroups per
// SIMD share the CU's 160 KB (the 92-VGPR one-fill kernels are register-good for five).
// "this robot still has its polish release" (Lane::iterate): bit 9 of the stance word in the hand-over records of a RUNNING robot
// (re-pack areas, the paired waves' list); inside a lane it is the sign of the lane's multiplier tolerance `tol_s`, and a fresh
// robot starts from DevParams::tol_start
constexpr uint32_t QC_POLISH_ONE = 1u << 9;
enum { IN_B = 0, IN_R = 6, IN_FLAGS = 18, IN_IDX = 19, IN_PLANES = 20,
       OUT_F = 0, OUT_STAT = 12, OUT_WORD = 13, OUT_IDX = 14, OUT_PLANES = 15,
       STOCK_PLANES = IN_PLANES + OUT_PLANES };
constexpr int stock_slots(int G) { return 64 / G; }
constexpr int TASK_DOUBLES = 32;  // 256 one-byte (robot, leg) tasks of the torque pass, behind the planes
constexpr int stock_doubles(int slots) { return ((STOCK_PLANES * (slots + 1) + TASK_DOUBLES + 63) / 64) * 64; }
// QPARK - the one-lane one-fill joint_q kernels of the 6x6 forms (round 6).  The torque pass needs every robot's twelve joint angles a
// second time, tens of microseconds after the fill read them - by then the wave's lines have left the XCD's 4 MB L2 (a resident round of
// workgroups streams 16 MB through it), so they came from the fabric again: 96 B per robot on top of the algorithmic bytes
// (profiles/r06b_tick_full262144: FETCH 1.15x).  They are parked in LDS instead, twelve planes next to the nine of Rwb.  The room: the
// re-pack records of the 4-lane tail move UNDER the output stock (nobody parks a result before the last record has been read:
// finish_on_four_lanes<HOLD>, and the lanes that finished on the one-lane body push after the tail), which frees the input-stock area:
//   [0, 9) Rwb   [9, 21) joint_q   [21, 36) output stock (= re-pack records during the tail)   + the task bytes
// 36 x 65 + 32 doubles = 19 KB: eight workgroups per CU still fit the 160 KB.
constexpr int QPARK_R = 0, QPARK_Q = 9, QPARK_OUT = 21, QPARK_PLANES = 36;
constexpr int qpark_doubles() { return ((QPARK_PLANES * 65 + TASK_DOUBLES + 63) / 64) * 64; }

// RACE (mode-2 kernels of batches that leave most SIMDs idle): several lane groups solve the SAME robot with
// different pivoting strategies and the first to reach the KKT point wins.  A strategy is (nclamp, drop_all):
// the first `nclamp` recalculations clamp f^ into the frusta keeping the faces already in the set (1 = the
// classic method; more = further projection steps before the first ratio test), and after a full step either the
// most negative multiplier is dropped or all negative ones at once.  Every strategy is a primal active-set method
// that stops only at the KKT point of the strictly convex QP, i.e. at the same minimiser.
template <class Eqp, bool KIN, bool RACE = false>
struct Lane {
  static constexpr int G = Eqp::G;
  static constexpr int FPL = 4 / G;  // feet per lane
  static constexpr bool S = Eqp::kStrided;
  // the state update of a recalculation on the packed working-set word (iterate): the strided 4-lane kernels, whose lone
  // wave pays every instruction of the recalculation on its serial chain
  static constexpr bool kPacked = S;
  static_assert(!kPacked || FPL == 1, "the packed update takes negbits in the working-set word's layout, which multipliers_ok builds only below FPL == 4");
  // ... and that word IS the lane's working-set state (the 6x6 forms' packed lanes): `wset` is carried from one recalculation
  // to the next, iterate() decodes the ints of `C` from it for the solve and writes only the word back, so `C` is scratch
  // inside iterate() there and everything outside reads and writes the state through set_foot_code() / foot_code()
  static constexpr bool kWord = kPacked && Eqp::kWordState;
  static_assert(!kWord || FPL == 1, "foot_code() / set_foot_code() hold the one foot of the lane: `wset` has no second field to keep");
  // ... whose face coefficients and force bounds come from the lane's FaceConst (uniform form)
  static constexpr bool kArith = kWord && Eqp::kFaceArith;
  // what the lane's tolerance carries on top of tol_d: the solve's scale factor, and for the kArith lanes, whose solve hands
  // over HALF the gradient (eqp_diagw, pass 2), half of that.  Every multiplier test compares a multiple of g with
  // tol_s x scale, so both sides are the parent's halved exactly and every decision is the same.  Whoever hands a lane a
  // robot sets tol_s with the RECEIVING lane's kTol.
  static constexpr double kTol = Eqp::kTolScale * (kArith ? 0.5 : 1.0);
  Wrench<FPL> Wr;
  Cube<FPL> C;
  double f[3 * FPL];
  long idx;
  uint32_t stance;  // bits 0-3: LegState per foot, bit 8: non-finite input
  int foot0;        // first foot of this lane
  int status, iters;
  double tol_s;  // relative multiplier tolerance of this robot (tol_d x kTol), signed: + while it still has its polish release, - after
  bool have_f;  // (read only by a MIXED recalculation without RACE, which no kernel runs; yet dropping its stores reshuffles the registers of most kernels)
  // the last recalculation was this robot's KKT point and the robot was live: what a racing group votes with.  It stands for
  // `busy & done & status == QC_SOLVED` only where the caller passes its `busy` as `live` and votes right after iterate() - all
  // three after() lambdas do (a live robot's status turns QC_SOLVED in exactly that recalculation); nothing else reads it
  bool kkt = false;
  int nclamp = 1;        // RACE: recalculations that clamp instead of stepping
  bool drop_all = false;  // RACE: drop every negative multiplier after a full step
  // kWord: the working-set word, this lane's foot at ITS place (bits 6 foot0 ... 6 foot0 + 5: the update's masks need no
  // shift).  Bits outside that field are whatever the group-uniform masks of past updates left there; readers take the field
  uint32_t wset = 0u;
  FaceConst fk = {0.0, 0.0, 0.0};  // kArith: set_face_const()

  // the six bits (encode_foot) of foot i of this lane
  QC_DEV uint32_t foot_code(int i) const {
    if constexpr (kWord) return (wset >> (6 * foot0)) & 63u;
    else return encode_foot(C.sx[i], C.sy[i], C.sz[i]);
  }
  // ... and their only writer outside iterate(); `code` holds valid fields (0, 1 or 3).  After foot0.
  QC_DEV void set_foot_code(int i, uint32_t code) {
    if constexpr (kWord) {
      wset = (code & 63u) << (6 * foot0);
    } else {
      C.sx[i] = dec2(code); C.sy[i] = dec2(code >> 2); C.sz[i] = dec2(code >> 4);
    }
  }
  // kArith: the foot's constants with its contact state folded in.  After stance and foot0, by whoever hands the lane a robot.
  template <class PT>
  QC_DEV void set_face_const(const PT& P) {
    if constexpr (kArith) {
      const bool st = (stance >> foot0) & 1u;
      fk.iw = st ? P.inv_w_u : 0.0;
      fk.lo = st ? P.fzmin : 0.0;
      fk.hi = st ? P.fzmax : 0.0;
    }
  }

  template <class PT>
  QC_DEV double lo(const PT& P, int i) const {
    if constexpr (kArith) return fk.lo;
    else return ((stance >> (foot0 + i)) & 1u) ? P.fzmin : 0.0;
  }
  template <class PT>
  QC_DEV double hi(const PT& P, int i) const {
    if constexpr (kArith) return fk.hi;
    else return ((stance >> (foot0 + i)) & 1u) ? P.fzmax : 0.0;
  }

  // multiplier test on the current face: true if all active faces have
  // lambda >= -tol; otherwise wcode = 3*foot+axis of the most negative one.
  // (`worst`: the smallest multiplier, face code in its low bits; `thr` = the bar below which a multiplier is released:
  // -tol |g|, or +tol |g| while the robot has its polish release - see iterate)
  template <class PT>
  QC_DEV bool multipliers_ok(const PT& P, const double (&g)[3 * FPL], double gscale, double& worst, double& thr, bool (&neg)[3 * FPL], uint32_t& negbits) const {
    negbits = 0u;
    // the tolerance is relative to the scale of the multipliers' rounding noise: what the 6x6 forms' solve hands over
    // (eqp_diagw: group-uniform, ready before the gradient is), max(1, |g|_inf) over the group's feet for the dense forms
    double gs = gscale;
    if constexpr (!Eqp::kHasScale) {
      gs = 1.0;
#pragma unroll
      for (int k = 0; k < 3 * FPL; k++) gs = max_abs_nn(gs, g[k]);
      gs = group_max<G, S>(gs);
    }
    thr = tol_s * gs;
    double cand[3 * FPL];
#pragma unroll
    for (int i = 0; i < FPL; i++) {
      const double lx = -(double)C.sx[i] * g[3 * i];
      const double ly = -(double)C.sy[i] * g[3 * i + 1];
      const double lz = (double)C.sz[i] * (P.mu * (lx + ly) - g[3 * i + 2]);
      const int c0 = 3 * (foot0 + i);
      // an inactive face: +BIG's high word over whatever low word (one select, as step_cand).  `worst` is read past `opt` only
      // when it is below the bar, which nothing with that high word is
      const double vx = big_unless(C.sx[i] != 0, lx), vy = big_unless(C.sy[i] != 0, ly), vz = big_unless(C.sz[i] != 0, lz);
      cand[3 * i + 0] = tag(vx, c0 + 0);
      cand[3 * i + 1] = tag(vy, c0 + 1);
      cand[3 * i + 2] = tag(vz, c0 + 2);
      if constexpr (RACE) {  // per-axis "this multiplier is negative" for the drop-all strategy (compares; the masks live in SGPRs)
        // on the selected value BEFORE its tag (the tag moves the low five bits): an active face's is its multiplier, an inactive
        // face's about 1e300 and under no bar
        neg[3 * i + 0] = vx < thr;
        neg[3 * i + 1] = vy < thr;
        neg[3 * i + 2] = vz < thr;
        if constexpr (FPL == 4) {
          // one lane per robot (the dense form's twin race): twelve lane masks = twelve SGPR pairs across the state update, next to a
          // kernel whose pointers already fill half of the SGPR file - they spill, and SGPR pairs that spill leave frame slots.
          // The same twelve answers as bits of one VGPR (negbits); the bool array is dead on this path.
          negbits |= (neg[3 * i + 0] ? 1u : 0u) << (3 * i) | (neg[3 * i + 1] ? 2u : 0u) << (3 * i) | (neg[3 * i + 2] ? 4u : 0u) << (3 * i);
          neg[3 * i + 0] = neg[3 * i + 1] = neg[3 * i + 2] = false;
        } else if constexpr (kPacked) {
          // packed state update (iterate): the answers as the release mask itself, both bits of every negative axis, at the
          // axis' place in the working-set word
          // (the three masks shifted to the foot's place: they do not change while the lane keeps its robot)
          const uint32_t sh = 6u * (uint32_t)(foot0 + i);
          negbits |= (neg[3 * i + 0] ? 3u << sh : 0u) | (neg[3 * i + 1] ? 12u << sh : 0u) | (neg[3 * i + 2] ? 48u << sh : 0u);
          neg[3 * i + 0] = neg[3 * i + 1] = neg[3 * i + 2] = false;
        }
      } else {
        neg[3 * i + 0] = neg[3 * i + 1] = neg[3 * i + 2] = false;
      }
    }
#pragma unroll
    for (int w = 3 * FPL; w > 1; w = (w + 1) / 2)
#pragma unroll
      for (int k = 0; k < w / 2; k++) cand[k] = min_nn(cand[k], cand[k + (w + 1) / 2]);
    worst = group_min<G, S>(cand[0]);
    return !(worst < thr);
  }

  // one working-set recalculation; returns true when the robot is finished.
  // PHASE: FIRST / STEADY - every robot of a wave is fresh in its first recalculation and none afterwards, so the
  // first is peeled and the steady body carries no clamp, no fresh/running selects and no ratio test for nothing.
  // MIXED: fresh and running robots share the wave - the racing lanes, whose strategy takes its first `nclamp`
  // recalculations as clamp steps (without RACE: until `have_f` is set) - in one straight-line body, the clamp
  // behind a wave-uniform branch.
  // `live`: the lane's robot is still running.  The strided 4-lane kernels iterate every lane through a
  // wave-uniform loop (MFMA sums read all 64 lanes), finished robots included: a finished robot recomputes
  // the same f^ from the same working set (idempotent), so only what must not move once it has finished -
  // working set, status, iteration count - is held back by `live`, instead of copying the whole lane state
  // and selecting it back.  Callers whose EXEC mask already excludes finished robots pass true.
  // What makes that sound (the invariants behind `live`):
  //  * a SOLVED robot is a fixed point: the same working set gives the same f^ bit for bit, no face blocks (every
  //    candidate is +BIG, alpha clamps to 1, beta = 0), so f = f^ is rewritten with the value it already holds;
  //  * a robot that is finished WITHOUT being solved (QC_NOT_PD, the iteration cap, a racing group whose partner won)
  //    does keep moving f while C stays frozen - and nobody reads that f: store_result() writes zero forces for every
  //    status other than QC_SOLVED, and a racing loser never pushes (the winner's group does);
  //  * the cap is tested per lane (`iters >= P.max_iter` in the return value), so it holds for robots that did not start
  //    together as well - the refilled lane groups of the paired-waves consumer, whose records carry their own count; in a
  //    one-fill wave all robots happen to reach it in the same recalculation.
  // tests/test_gpu_matrix.py::test_iteration_cap_and_bad_inputs_agree_across_widths holds status, iteration count and the
  // (zero) forces of capped / bad robots equal across the lane-group widths.
  enum { MIXED = 0, FIRST = 1, STEADY = 2 };
  // the equality-constrained solve on the current face (kArith: with the lane's FaceConst)
  template <class PT>
  QC_DEV bool solve_face(const PT& P, Eqp& eqp, double (&fh)[3 * FPL], double (&g)[3 * FPL]) {
    if constexpr (kArith) return eqp.solve_arith(P, Wr, C, stance, foot0, fh, g, fk);
    else return eqp.solve(P, Wr, C, stance, foot0, fh, g);
  }
  // `empty_set` (wave-uniform): every robot of the wave still has the EMPTY working set - the first recalculation of a cold
  // fill.  With no active face there is no multiplier to test (every candidate is +BIG), so the test is skipped.
  template <int PHASE, class PT>
  QC_DEV bool iterate(const PT& P, Eqp& eqp, const bool live = true, const bool empty_set = false) {
    double fh[3 * FPL], g[3 * FPL];
    iters += live ? 1 : 0;
    if constexpr (kWord) {  // the solve's ints from the word's fields
      const uint32_t sh = 6u * (uint32_t)foot0;
      C.sx[0] = __builtin_amdgcn_sbfe((int)wset, sh, 2);
      C.sy[0] = __builtin_amdgcn_sbfe((int)wset, sh + 2, 2);
      C.sz[0] = __builtin_amdgcn_sbfe((int)wset, sh + 4, 2);
    }
    const bool pd = solve_face(P, eqp, fh, g);
    // RACE, MIXED: the lane's strategy decides (its first `nclamp` recalculations are clamp steps)
    const bool fresh = PHASE == FIRST ? true : (PHASE == STEADY ? false : (RACE ? iters <= nclamp : !have_f));
    have_f = true;
    // (a) fresh robot: clamp f^ into the frusta.  In MIXED recalculations the whole block sits behind a
    // wave-uniform branch: once every strategy is past its clamp steps nobody takes it.
    double fc[3 * FPL];
    Cube<FPL> Cc;
    bool changed = false;
#pragma unroll
    for (int i = 0; i < FPL; i++) {
      fc[3 * i] = fh[3 * i]; fc[3 * i + 1] = fh[3 * i + 1]; fc[3 * i + 2] = fh[3 * i + 2];
      Cc.sx[i] = Cc.sy[i] = Cc.sz[i] = 0;
    }
    if (PHASE == FIRST || (PHASE == MIXED && __builtin_amdgcn_ballot_w64(fresh) != 0)) {
      int ch = 0;
#pragma unroll
      for (int i = 0; i < FPL; i++)
        ch |= (int)clamp_foot(P.mu, lo(P, i), hi(P, i), C.sx[i], C.sy[i], C.sz[i], fc[3 * i], fc[3 * i + 1], fc[3 * i + 2], Cc.sx[i], Cc.sy[i],
                              Cc.sz[i]);
      changed = group_or<G, S>(ch) != 0;
    }
    // (b) otherwise: ratio test over the faces outside the working set (tree min, face code in the low bits)
    bool blocked = false;
    int bcode = -1;
    uint32_t alo = 0u;  // (kPacked: the low word of the smallest ratio - its face code)
    if constexpr (PHASE != FIRST) {
      // e = f - f^ is the step's operand below, and the directions are its negation (a source modifier): -(f - f^) is f^ - f bit
      // for bit, except that equal operands give -0 where the difference gives +0 - a zero direction, with which no face can
      // block (nd > eps fails) and whose sign no slack sees.  The step itself must keep e: fma(beta, -0, f^) turns a f^ of -0
      // into -0 where e = +0 gives +0.
      double cand[5 * FPL], e[3 * FPL];
#pragma unroll
      for (int i = 0; i < FPL; i++) {
        const double fx = f[3 * i], fy = f[3 * i + 1], fz = f[3 * i + 2];
        e[3 * i] = fx - fh[3 * i]; e[3 * i + 1] = fy - fh[3 * i + 1]; e[3 * i + 2] = fz - fh[3 * i + 2];
        const double dx = -e[3 * i], dy = -e[3 * i + 1], dz = -e[3 * i + 2];
        const double m = P.mu * fz, md = P.mu * dz;
        const bool zf = C.sz[i] == 0, xf = C.sx[i] == 0, yf = C.sy[i] == 0;
        const int c0 = 6 * (foot0 + i);
        cand[5 * i + 0] = step_cand(xf, m + fx, -dx - md, c0 + 0);     // X-
        cand[5 * i + 1] = step_cand(xf, m - fx, dx - md, c0 + 1);      // X+  (both X faces can block at once: mu dz < -|dx|)
        cand[5 * i + 2] = step_cand(yf, m + fy, -dy - md, c0 + 2);     // Y-
        cand[5 * i + 3] = step_cand(yf, m - fy, dy - md, c0 + 3);      // Y+
        cand[5 * i + 4] = step_cand_z(zf, fz, dz, lo(P, i), hi(P, i), c0 + 4);  // Z- (code c0 + 4) or Z+ (c0 + 5)
      }
#pragma unroll
      for (int w = 5 * FPL; w > 1; w = (w + 1) / 2)
#pragma unroll
        for (int k = 0; k < w / 2; k++) cand[k] = min_nn(cand[k], cand[k + (w + 1) / 2]);
      const double amin = group_min<G, S>(cand[0]);
      blocked = !fresh & (amin < 1.0e299);
      bcode = blocked ? tag_code(amin) : -1;
      alo = (uint32_t)__double_as_longlong(amin);
      // f <- f^ + (1 - alpha)(f - f^): exactly f^ for a full step.  No face blocks: amin = +BIG, clamped to alpha = 1
      // (branch-free; a blocking ratio that the approximate reciprocal rounds up to 1 is clamped too)
      const double beta = 1.0 - min_nn(max_nn(amin, 0.0), 1.0);
#pragma unroll
      for (int k = 0; k < 3 * FPL; k++) f[k] = fresh ? fc[k] : __builtin_fma(beta, e[k], fh[k]);
    } else {
#pragma unroll
      for (int k = 0; k < 3 * FPL; k++) f[k] = fc[k];
    }
    // multiplier test, meaningful when f landed on f^
    const bool at_fh = fresh ? !changed : !blocked;
    bool neg[3 * FPL];
#pragma unroll
    for (int k = 0; k < 3 * FPL; k++) neg[k] = false;
    bool opt = true;
    uint32_t negbits = 0u;  // (FPL == 4 && RACE: `neg` as bits of one register)
    double worst = QC_BIG, thr = 0.0;
    if (!(PHASE == FIRST && empty_set)) opt = multipliers_ok(P, g, eqp.gscale, worst, thr, neg, negbits);
    if constexpr (RACE && FPL == 4) asm volatile("" : "+v"(negbits));
    // POLISH.  The bar -tol |g| sits just above the multipliers' rounding noise, and along a weakly active face the objective
    // curves only with 2w: a multiplier accepted anywhere in (-tol |g|, 0) leaves the force up to tol |g| / (2w) from the
    // minimiser (w ~ 1e-7: 3e-3 N = 6.9e-5 relative, profiles/r05_fuzz_dig_138.log), and one whose true value is negative but
    // inside the noise about as far.  So a robot starts with the bar at +tol |g| (`thr` = tol_s x scale, tol_s > 0): a face
    // whose multiplier lies inside the band (-tol |g|, +tol |g|) counts as not optimal and is released like a negative one, and
    // the walk goes on as the primal active-set method it is (the objective never increases) - either the larger subproblem's
    // minimiser is feasible, which is the better point, or the released face blocks at a zero-length step and comes back.
    // The first release that was NOT of a clearly negative multiplier (|worst| <= tol |g|) flips the robot's tolerance for good:
    // from then on the rule is round 5's, so a weakly active face is released once and cannot cycle.  Clearly negative
    // multipliers are dropped as ever and leave the polish release in place.  Per recalculation: one compare and one select
    // (a budget counter in a register of its own cost the chain-bound kernels 2 %, the flag inside `status` 2.7 %, an EXEC
    // branch around the test 2-4.5 %: profiles/r06_polish_ab.log).
    const int wcode = (at_fh & !opt) ? tag_code(worst) : -1;
    {
      const bool polish = at_fh & !opt & (__builtin_fabs(worst) <= __builtin_fabs(thr));  // (false once tol_s < 0: then !opt means worst < -tol |g|)
      const unsigned long long tb = (unsigned long long)__double_as_longlong(tol_s);
      const uint32_t hi = (uint32_t)(tb >> 32) | (polish ? 0x80000000u : 0u);  // (select between constants: written as a select between the two words it became an EXEC branch)
      tol_s = __longlong_as_double((long long)(((unsigned long long)hi << 32) | (uint32_t)tb));
    }
    const bool dall = RACE & drop_all & at_fh;  // this lane's strategy drops every multiplier below the bar at once
    const bool take_clamp = fresh & changed;
    if constexpr (kPacked) {
      // The same update on the working-set word: two bits per axis (encode_foot: 0 free, 1 upper face, 3 = -1 lower face), six
      // per foot, foot k at bit 6 k - the layout of the warm-start word, in which a release code c = 3 foot + axis names the field
      // at bit 2 c and a blocking code c = 6 foot + 2 axis + (upper) the field at bit c & ~1.  A lane holds the fields of its own
      // feet and reads only those back, so masks that name another lane's field pass through unnoticed.  What the select chains
      // per axis decided is decided here by the same conditions: release (one field, or the strategy's negbits), then the
      // blocking face over it, then the clamp's set, then `live`.  Per recalculation that is a dozen integer instructions behind
      // the two reduced doubles instead of about fifty compares and selects.
      const uint32_t sh0 = 6u * (uint32_t)foot0;
      uint32_t w = 0u, wc = 0u;
#pragma unroll
      for (int i = 0; i < FPL; i++) {
        if constexpr (!kWord) w |= encode_foot(C.sx[i], C.sy[i], C.sz[i]) << (6 * i);
        if constexpr (PHASE != STEADY) wc |= encode_foot(Cc.sx[i], Cc.sy[i], Cc.sz[i]) << (6 * i);
      }
      w <<= sh0;
      if constexpr (kWord) w = wset;  // carried, not re-encoded
      const uint32_t wlo = (uint32_t)__double_as_longlong(worst);
      const uint32_t rel1 = (at_fh & !opt) ? 3u << (((wlo & 31u) << 1) & 31u) : 0u;
      const uint32_t rel = RACE ? (dall ? negbits : rel1) : rel1;
      uint32_t nw = w & ~rel;
      if constexpr (PHASE != FIRST) {
        const uint32_t field = 3u << (alo & 30u);
        const uint32_t val = field ^ ((alo & 1u) << (alo & 31u));  // upper face (odd code): 1, lower: 3
        const uint32_t bm = blocked ? field : 0u;
        nw = (nw & ~bm) | (val & bm);
      }
      if constexpr (PHASE != STEADY) nw = take_clamp ? wc << sh0 : nw;
      nw = live ? nw : w;
      if constexpr (kWord) {
        wset = nw;
      } else {
#pragma unroll
        for (int i = 0; i < FPL; i++) {
          C.sx[i] = __builtin_amdgcn_sbfe((int)nw, sh0 + 6 * i, 2);
          C.sy[i] = __builtin_amdgcn_sbfe((int)nw, sh0 + 6 * i + 2, 2);
          C.sz[i] = __builtin_amdgcn_sbfe((int)nw, sh0 + 6 * i + 4, 2);
        }
      }
    } else {
#pragma unroll
    for (int i = 0; i < FPL; i++) {
      int sx = C.sx[i], sy = C.sy[i], sz = C.sz[i];
      const int b0 = 6 * (foot0 + i), w0 = 3 * (foot0 + i);
      const bool nx = (RACE && FPL == 4) ? ((negbits >> (3 * i)) & 1u) != 0 : neg[3 * i + 0];
      const bool ny = (RACE && FPL == 4) ? ((negbits >> (3 * i + 1)) & 1u) != 0 : neg[3 * i + 1];
      const bool nz = (RACE && FPL == 4) ? ((negbits >> (3 * i + 2)) & 1u) != 0 : neg[3 * i + 2];
      const bool px = RACE ? (dall ? nx : wcode == w0 + 0) : wcode == w0 + 0;
      const bool py = RACE ? (dall ? ny : wcode == w0 + 1) : wcode == w0 + 1;
      const bool pz = RACE ? (dall ? nz : wcode == w0 + 2) : wcode == w0 + 2;
      sx = (bcode == b0 + 0) ? -1 : ((bcode == b0 + 1) ? 1 : (px ? 0 : sx));
      sy = (bcode == b0 + 2) ? -1 : ((bcode == b0 + 3) ? 1 : (py ? 0 : sy));
      sz = (bcode == b0 + 4) ? -1 : ((bcode == b0 + 5) ? 1 : (pz ? 0 : sz));
      C.sx[i] = live ? (take_clamp ? Cc.sx[i] : sx) : C.sx[i];
      C.sy[i] = live ? (take_clamp ? Cc.sy[i] : sy) : C.sy[i];
      C.sz[i] = live ? (take_clamp ? Cc.sz[i] : sz) : C.sz[i];
    }
    }
    // (bitwise on purpose: short-circuit forms become exec-mask branches on the serial chain)
    const bool solved = pd & at_fh & opt;
    kkt = live & solved;  // (a live robot's status is QC_SOLVED exactly when it has just been solved: the vote needs no look at `status`)
    status = live ? (!pd ? (int)QC_NOT_PD : (solved ? (int)QC_SOLVED : status)) : status;  // otherwise it stays QC_MAX_ITER
    return (!pd) | solved | (iters >= P.max_iter);
  }

  // take the robot staged in `slot` of the wave's input stock into this lane's group
  // (`tol` = DevParams::tol_start: a fresh robot has its polish release unless the handle switched the polish off)
  template <int SP>
  QC_DEV void load_from_stock(const double* __restrict__ sin, int slot, int member, double tol) {
    foot0 = member * FPL;
#pragma unroll
    for (int k = 0; k < 6; k++) {
      Wr.b[k] = Eqp::kNegB ? -sin[(IN_B + k) * SP + slot] : sin[(IN_B + k) * SP + slot];
      // (opaque: otherwise the compiler keeps +b and re-materialises the negation - an MFMA addend takes no source
      // modifier - inside every recalculation)
      if constexpr (Eqp::kNegB) asm volatile("" : "+v"(Wr.b[k]));
    }
#pragma unroll
    for (int i = 0; i < FPL; i++)
#pragma unroll
      for (int k = 0; k < 3; k++) Wr.r[i][k] = sin[(IN_R + 3 * (foot0 + i) + k) * SP + slot];
    const unsigned long long fl = (unsigned long long)__double_as_longlong(sin[IN_FLAGS * SP + slot]);
    stance = (uint32_t)fl;
    tol_s = kTol * tol;
    const uint32_t wv = (uint32_t)(fl >> 32);
    idx = __double_as_longlong(sin[IN_IDX * SP + slot]);
    const bool use_warm = (wv & 0x80000000u) != 0;
#pragma unroll
    for (int i = 0; i < FPL; i++) {
      const uint32_t fb = wv >> (6 * (foot0 + i));
      const bool st = use_warm && ((stance >> (foot0 + i)) & 1u);
      if constexpr (kWord) {
        // (a caller's word may hold the unused field value 2, which dec2 reads as free: keep a field only if its bit 0 is set)
        const uint32_t b0 = fb & 0x15u;
        set_foot_code(i, st ? (fb & (b0 | (b0 << 1))) : 0u);
      } else {
        C.sx[i] = st ? dec2(fb) : 0;
        C.sy[i] = st ? dec2(fb >> 2) : 0;
        C.sz[i] = st ? dec2(fb >> 4) : 0;
      }
    }
#pragma unroll
    for (int k = 0; k < 3 * FPL; k++) f[k] = 0.0;
    status = QC_MAX_ITER;
    iters = 0;
    have_f = false;
  }

  // take a freshly assembled robot straight from registers (one lane per robot, no stock in between)
  QC_DEV void load_direct(const Wrench<FPL>& W, uint32_t st, uint32_t wv, long robot, int member, double tol) {
    static_assert(G == 1, "one lane assembles and solves the whole robot");
    foot0 = member * FPL;
#pragma unroll
    for (int k = 0; k < 6; k++) {
      Wr.b[k] = Eqp::kNegB ? -W.b[k] : W.b[k];
      if constexpr (Eqp::kNegB) asm volatile("" : "+v"(Wr.b[k]));
    }
#pragma unroll
    for (int i = 0; i < FPL; i++)
#pragma unroll
      for (int k = 0; k < 3; k++) Wr.r[i][k] = W.r[i][k];
    stance = st;
    tol_s = kTol * tol;
    idx = robot;
    const bool use_warm = (wv & 0x80000000u) != 0;
#pragma unroll
    for (int i = 0; i < FPL; i++) {
      const uint32_t fb = wv >> (6 * (foot0 + i));
      const bool on = use_warm && ((stance >> (foot0 + i)) & 1u);
      C.sx[i] = on ? dec2(fb) : 0;
      C.sy[i] = on ? dec2(fb >> 2) : 0;
      C.sz[i] = on ? dec2(fb >> 4) : 0;
    }
#pragma unroll
    for (int k = 0; k < 3 * FPL; k++) f[k] = 0.0;
    status = QC_MAX_ITER;
    iters = 0;
    have_f = false;
  }
  // bit 9 of the stance word a RUNNING robot travels with (hand-over records)
  QC_DEV uint32_t polish_bit() const { return tol_s > 0.0 ? QC_POLISH_ONE : 0u; }
  // the working-set word of this lane's feet (bit 31 = valid is added by the caller)
  QC_DEV uint32_t word_bits() const {
    uint32_t word = 0;
#pragma unroll
    for (int i = 0; i < FPL; i++) word |= foot_code(i) << (6 * (foot0 + i));
    return word;
  }

  // park the finished robot's result in `slot` of the wave's output stock
  template <int SP>
  QC_DEV void push_result(double* __restrict__ sout, int slot) const {
    uint32_t word = 0;
#pragma unroll
    for (int i = 0; i < FPL; i++) {
#pragma unroll
      for (int k = 0; k < 3; k++) sout[(OUT_F + 3 * (foot0 + i) + k) * SP + slot] = f[3 * i + k];
      word |= foot_code(i) << (6 * (foot0 + i));
    }
    word = (uint32_t)group_or<G, S>((int)word) | 0x80000000u;
    if (foot0 == 0) {
      sout[OUT_STAT * SP + slot] = __longlong_as_double((long long)(((unsigned long long)(uint32_t)iters << 32) | (uint32_t)status));
      sout[OUT_WORD * SP + slot] = __longlong_as_double((long long)(((unsigned long long)stance << 32) | word));
      sout[OUT_IDX * SP + slot] = __longlong_as_double(idx);
    }
  }
};

// One working-set recalculation with the constants where the loop keeps them.  RESIDENT: a register copy (UConst), loaded
// once here and pinned before every recalculation - no scalar load + wait per recalculation; otherwise the constant buffer,
// re-derived at every recalculation (QC_PARAMS_HERE).
template <bool RESIDENT>
struct Recalc {
  const DevParams* Pg;
  UConst uc;
  QC_DEV explicit Recalc(const DevParams* pg) : Pg(pg) {
    if constexpr (RESIDENT) uc = load_uconst(*QC_PARAMS_HERE(Pg));
  }
  template <int PHASE, class LaneX, class EqpX>
  QC_DEV bool step(LaneX& lane, EqpX& eqp, const bool live, const bool empty_set = false) {
    if constexpr (RESIDENT) {
      pin_uconst(uc);
      return lane.template iterate<PHASE>(uc, eqp, live, empty_set);
    } else {
      return lane.template iterate<PHASE>(*QC_PARAMS_HERE(Pg), eqp, live, empty_set);
    }
  }
};

// The votes of the lane groups racing on one robot, ORed together: N groups, ROT lanes apart within their row of 16.
template <int ROT, int N>
QC_DEV int race_or(const int mine) {
  int m = mine | __builtin_amdgcn_update_dpp(0, mine, 0x120 + ROT, 0xF, 0xF, true);  // row_ror by ROT lanes: the partner groups
  if constexpr (N == 4) {
    m |= __builtin_amdgcn_update_dpp(0, mine, 0x120 + 2 * ROT, 0xF, 0xF, true);
    m |= __builtin_amdgcn_update_dpp(0, mine, 0x120 + 3 * ROT, 0xF, 0xF, true);
  }
  return m;
}

// Dense phases around the divergent solve.  Robots need 1 ... ~20
// recalculations, so the solver lanes are refilled a few at a time; running the
// expensive per-robot assembly (rotation log with atan2/sqrt, Newton-Euler
// right-hand side, optional forward kinematics: ~1400 instructions) and the
// output transform under such sparse exec masks would waste most of the wave.
// Instead every LANE assembles one whole robot for a stock of 64 robots in LDS,
// groups pull from the stock with a handful of ds_reads, finished groups push
// their world-frame forces to an output stock, and a dense pass (again one robot
// per lane) rotates them to the body frame, applies J^T and stores.
// Stock planes are [field][64 slots] doubles: the dense side touches
// plane[field][lane] (conflict-free), the group side one slot per group.
// Swing-planning state update of one robot at the start of its tick, commander_node.cpp:432-471:
// FootPlanner::updateStates (foot_planner.cpp:106-157) decides which legs need a new foothold (stance ->
// swing edge, or any swinging leg on the very first call); if there is one, FootTrajectoryManager::
// referenceStates(gait_map, bounds) (trajectory.cpp:308-344) CLEARS every stored trajectory and creates
// those of the planned legs from p_start = Rwb foot + x (commander_node.cpp:456) and the planned foothold.
// Returns the has_traj bits of this lane's legs after the update (bit = leg number): they travel in the robot's stance word (bits
// 12-15) to the torque pass, which used to read them back - one agent-scope load per swing leg, of a record line the wave
// already had - from memory.
template <int FPL, bool STR = false>
QC_DEV uint32_t swing_plan(CParams& P, const BatchIn& in, long robot, int foot0, uint32_t stance, const RawState& St, const Wrench<FPL>& W,
                           const TickExtra& X) {
  constexpr int GG = 4 / FPL;
  SwingState* S = in.swing_state + robot;
  const bool first = X.leg_state[0] < 0;  // state_map_.empty()
  int plan = 0;
  int had[FPL];
#pragma unroll
  for (int i = 0; i < FPL; i++) {
    // (selects over the four fetched words: foot0 is a per-lane value in the lane-group layouts)
    const int f = foot0 + i;
    const int prev = f == 0 ? X.leg_state[0] : (f == 1 ? X.leg_state[1] : (f == 2 ? X.leg_state[2] : X.leg_state[3]));
    had[i] = f == 0 ? X.has[0] : (f == 1 ? X.has[1] : (f == 2 ? X.has[2] : X.has[3]));
    const bool swing_now = !((stance >> f) & 1u);
    if (swing_now && (first || prev == 1)) plan |= 1 << i;
  }
  const bool any = group_or<GG, STR>(plan) != 0;
  uint32_t has_bits = 0u;
#pragma unroll
  for (int i = 0; i < FPL; i++) {
    const int leg = foot0 + i;
    if ((plan >> i) & 1) {
      // foot_actual_map (commander_node.cpp:383-384) went through Rwb in the wrench assembly already: W.r[i] = Rwb foot_body
      double fh[3];
      plan_foothold(P, leg, St.R, St.x, St.xdot, St.w, St.xdotd, W.r[i], fh);
#pragma unroll
      for (int r = 0; r < 3; r++) {
        S->p_start[3 * leg + r] = W.r[i][r] + St.x[r];  // Rwb foot + x, :456
        S->p_final[3 * leg + r] = fh[r];
      }
    }
    const int has_now = any ? ((plan >> i) & 1) : had[i];
    S->has_traj[leg] = has_now;
    S->leg_state[leg] = ((stance >> leg) & 1u) ? 1 : 0;
    has_bits |= has_now ? (1u << leg) : 0u;
  }
  return has_bits;
}

// the assembly of one robot (or of this lane's feet of it): wrench target and lever arms, contact state, optional
// gait clock and swing planning.  Returns the stance word (bits 0-3 LegState, bit 8 = non-finite input).
// (`S`, `fp`: what fetch_state() read - in commander mode the step may replace its desired state; `sw`: the robot's four
// LegState bytes if in.stance is given)
template <bool KIN, int FPL, bool STR>
QC_DEV uint32_t assemble_from_state(CParams& P, const BatchIn& in, long robot, int member, RawState& S, const double (&fp)[3 * FPL], uint32_t sw,
                                    const TickExtra& X, Wrench<FPL>& W) {
  constexpr int GG = 4 / FPL;
  const int foot0 = member * FPL;
  // commander mode: until the gait runs, make_stance_gait() with the phases held and no planning (commander_node.cpp:366, 480)
  const bool run = !(KIN && in.cmd_state) || commander_step(in, robot, member, S, X);
  const double fin = wrench_from_state<FPL, KIN>(P, S, fp, foot0, W);
  uint32_t stance = 0xFu;  // make_stance_gait(), gait.cpp:24-34
  if (in.stance) {
    stance = ((sw & 0xFFu) ? 1u : 0u) | ((sw & 0xFF00u) ? 2u : 0u) | ((sw & 0xFF0000u) ? 4u : 0u) | ((sw & 0xFF000000u) ? 8u : 0u);
  } else if (in.gait_phase && run) {
    // GaitScheduler::phase(): phase_in_stance (qc_device.hpp)
    const double duty = in.gait_duty ? X.duty : P.stance_phase;
    stance = 0;
    double phs[4];
#pragma unroll
    for (int i = 0; i < 4; i++) phs[i] = X.ph[i];
    if (in.gait_dt) {  // GaitScheduler::update(dt), gait.cpp:113-123: the clock of this robot advances first
      const double step = gait_clock_step(P, X.dt);
      double* wp = in.gait_phase + 4 * robot;
#pragma unroll
      for (int i = 0; i < 4; i++) {
        phs[i] = advance_phase(phs[i], step);  // (qc_device.hpp: fmod(v, 1.0) bit for bit)
        // every lane of the group computes the same four values; the first one stores them (read again by this wave's
        // store phase for the swing trajectories - workgroup scope, see swing_fetch)
        if (member == 0) __hip_atomic_store(wp + i, phs[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      }
    }
#pragma unroll
    for (int i = 0; i < 4; i++) stance |= phase_in_stance(phs[i], duty) ? (1u << i) : 0u;
  }
  if (KIN && in.swing_state && run)  // (bits 12-15: has_traj per leg, for the torque pass; only member 0's word reaches the stock: the group's bits are or-ed)
    stance |= (uint32_t)group_or<GG, STR>((int)swing_plan<FPL, STR>(P, in, robot, foot0, stance, S, W, X)) << 12;
  // non-finite inputs poison b, r or R: report QC_NOT_PD instead of iterating on NaNs
  const bool bad = group_or<GG, STR>(!(fin == 0.0) ? 1 : 0) != 0;
  if (bad) {
    stance |= 0x100u;
#pragma unroll
    for (int k = 0; k < 6; k++) W.b[k] = 0.0;
#pragma unroll
    for (int i = 0; i < FPL; i++) W.r[i][0] = W.r[i][1] = W.r[i][2] = 0.0;
  }
  return stance;
}

template <bool KIN, int FPL, bool STR>
QC_DEV uint32_t assemble_robot(CParams& P, const BatchIn& in, long robot, int member, Wrench<FPL>& W) {
  // all loads first, back to back (see the one-lane fill in balance_kernel): one memory round trip instead of four
  const uint32_t sw = in.stance ? *reinterpret_cast<const uint32_t*>(in.stance + 4 * robot) : 0u;
  RawState S;
  TickExtra X;
  double fp[3 * FPL];
  fetch_extra<KIN>(in, robot, X);
  fetch_state<FPL, KIN>(in, robot, member * FPL, S, fp);
  asm volatile("" ::: "memory");
  return assemble_from_state<KIN, FPL, STR>(P, in, robot, member, S, fp, sw, X, W);
}

// FPL = 4: one lane assembles a whole robot (dense restock of a big batch);
// FPL = 4/G: the G lanes of a group share a robot, each doing its own feet
// (small fills, where latency matters more than lane efficiency).
template <bool KIN, int FPL, bool STR, int SP>
QC_DEV void assemble_to_stock(CParams& P, const BatchIn& in, const uint32_t* __restrict__ warm, long robot, int slot, int member,
                              double* __restrict__ sin) {
  Wrench<FPL> W;
  const int foot0 = member * FPL;
  const uint32_t wv = warm ? warm[robot] : 0u;  // (issued with the robot's other loads, not behind the assembly)
  const uint32_t stance = assemble_robot<KIN, FPL, STR>(P, in, robot, member, W);
#pragma unroll
  for (int i = 0; i < FPL; i++)
#pragma unroll
    for (int k = 0; k < 3; k++) sin[(IN_R + 3 * (foot0 + i) + k) * SP + slot] = W.r[i][k];
  if (member == 0) {
#pragma unroll
    for (int k = 0; k < 6; k++) sin[(IN_B + k) * SP + slot] = W.b[k];
    sin[IN_FLAGS * SP + slot] = __longlong_as_double((long long)(((unsigned long long)wv << 32) | stance));
    sin[IN_IDX * SP + slot] = __longlong_as_double(robot);
  }
}

// output transform, BC.cpp:218-232: fb = -Rwb^T fw for stance legs.  `fw` = world-frame forces of
// the FPL feet from foot0 on; `member` 0 also writes the per-robot words.  (The joint torques of the widened tick are the
// torque pass's, below.)
// `Rl` != nullptr: the robot's Rwb is parked in LDS (entry k at Rl[k * rstride]) by the wave's assembly phase - the one-lane
// one-fill kernel keeps it there instead of reading the 72-byte row from global memory a second time.
// (RLDS is a template parameter, not a null test on `Rl`: a load through a pointer selected between LDS and global memory is
// a FLAT load - it was one, nine times per robot, in every one-lane kernel of rounds 2 and 3.)
template <bool KIN, int FPL, bool RLDS = false>
QC_DEV void store_result(CParams& P, const BatchIn& in, const BatchOut& out, long idx, uint32_t stance, int status, int iters, uint32_t word,
                         const double (&fw)[3 * FPL], int member, const double* __restrict__ Rl = nullptr, int rstride = 0) {
  const int foot0 = member * FPL;
  double R[9];
  if constexpr (RLDS) {
#pragma unroll
    for (int k = 0; k < 9; k++) R[k] = Rl[k * rstride];
  } else {
    const double* Rp = in.Rwb + 9 * idx;
#pragma unroll
    for (int k = 0; k < 9; k++) R[k] = Rp[k];
  }
  const int st_out = (stance & 0x100u) ? (int)QC_NOT_PD : status;
  double* o = out.grf_body + 12 * idx + 3 * foot0;
#pragma unroll
  for (int i = 0; i < FPL; i++) {
    const bool st = ((stance >> (foot0 + i)) & 1u) && st_out == QC_SOLVED;
    double f[3];
#pragma unroll
    for (int k = 0; k < 3; k++) f[k] = fw[3 * i + k];
#pragma unroll
    for (int r = 0; r < 3; r++) {
      const double v = -(R[r] * f[0] + R[3 + r] * f[1] + R[6 + r] * f[2]);
      o[3 * i + r] = st ? v : 0.0;
    }
  }
  if (member == 0) {
    out.status[idx] = st_out;
    if (out.active_set) out.active_set[idx] = word;
    if (out.iterations) out.iterations[idx] = iters;
  }
}

template <bool KIN, int FPL, int SP, bool RLDS = false>
QC_DEV void store_from_stock(CParams& P, const BatchIn& in, const BatchOut& out, const double* __restrict__ sout, int slot, int member,
                             const double* __restrict__ Rl = nullptr) {
  const int foot0 = member * FPL;
  const long idx = __double_as_longlong(sout[OUT_IDX * SP + slot]);
  const unsigned long long sw = (unsigned long long)__double_as_longlong(sout[OUT_STAT * SP + slot]);
  const unsigned long long ww = (unsigned long long)__double_as_longlong(sout[OUT_WORD * SP + slot]);
  double fw[3 * FPL];
#pragma unroll
  for (int k = 0; k < 3 * FPL; k++) fw[k] = sout[(OUT_F + 3 * foot0 + k) * SP + slot];
  store_result<KIN, FPL, RLDS>(P, in, out, idx, (uint32_t)(ww >> 32), (int)(uint32_t)sw, (int)(uint32_t)(sw >> 32), (uint32_t)ww, fw, member, Rl, SP);
}

// dense assembly of the next (up to 64) robots of the chunk into the input stock; returns how many
template <int G, bool KIN, bool STR, int SP>
QC_DEV int restock(const DevParams* __restrict__ Pg, const BatchIn& in, const uint32_t* __restrict__ warm, long cursor, long end, int lane,
                   int member, double* __restrict__ sin) {
  const long left = end - cursor;
  const int k = left < 64 ? (int)left : 64;
  if (G > 1 && k <= 64 / G) {  // few robots: the lanes of a group share one
    const int grp = lane_group<G, STR>(lane);
    if (grp < k) {
      CParams& P = *QC_PARAMS_HERE(Pg);
      assemble_to_stock<KIN, 4 / G, STR, SP>(P, in, warm, cursor + grp, grp, member, sin);
    }
  } else if (lane < k) {
    CParams& P = *QC_PARAMS_HERE(Pg);
    assemble_to_stock<KIN, 4, false, SP>(P, in, warm, cursor + lane, lane, 0, sin);
  }
  __syncthreads();
  return k;
}

// ---- the torque pass of the widened tick (SURVEY 8f rows 1 + 4): joint_tau of the robots parked in the output stock ----------
// commander_node.cpp:482-531: swing legs get IK -> J^-1 -> joint PD torques, stance legs tau = J^T f_body, all clamped.
// Round 3 looped over the four legs with one robot per lane and a per-lane `if (swing) ... else ...`: in a batch of mixed
// contact states every leg is swinging in SOME lane, so every lane walked through IK + J^-1 + PD and through J^T four times.
// Now a swinging (robot, leg) pair is a TASK: the wave's swing tasks are listed (one byte each: slot << 2 | leg, in a 256-byte
// array behind the stock planes; built with ballots and mbcnt, leg-major, so neighbouring lanes still touch neighbouring
// robots) and run in consecutive lanes - one or two passes of the ~650-instruction swing chain instead of four.  The cheap
// stance map (J^T f: three sincos and a dozen products per leg) stays one robot per lane: its loads are one coalesced batch and
// its per-leg constants scalar operands.
// What makes the pass cheap is as much WHEN its loads are issued (a wave of a one-round launch has its SIMD to itself: a
// dependent global load is ~1 us of nothing): the stance legs' joint angles are requested before the force stores, the first
// swing pass's inputs before the stance legs are computed, and every further swing pass's inputs while the previous one computes.
QC_DEV void store_tau(CParams& P, const BatchOut& out, long idx, int leg, const double (&tau)[3], bool emit) {
  double* to = out.joint_tau + 12 * idx + 3 * leg;
#pragma unroll
  for (int r = 0; r < 3; r++) {
    // arma::clamp (commander_node.cpp:526) is two compares: a NaN torque (NaN joint state) stays NaN, as in
    // the reference, instead of turning into a full-scale command the way fmin(fmax()) would make it
    const double t = tau[r];
    to[r] = emit ? (t < P.tau_min ? P.tau_min : (t > P.tau_max ? P.tau_max : t)) : 0.0;
  }
}
// what one swing-leg task reads from memory
struct SwingIn {
  long idx;
  int leg, has;
  double q[3], qdot[3], x[3], a[3], b[3], ph;  // a, b: trajectory end points (swing_state) or reference position / velocity (swing_pos / swing_vel)
};
// (`stance_word`: the robot's stance word from the output stock - bits 12-15 carry has_traj as the assembly phase left it)
// (`qslot` != nullptr - QPARK: the robot's parked joint angles, entry k at qslot[k * qstride])
QC_DEV void swing_fetch(const BatchIn& in, long idx, int leg, uint32_t stance_word, SwingIn& T, const double* __restrict__ qslot = nullptr, int qstride = 0) {
  T.idx = idx;
  T.leg = leg;
  T.has = 1;
  T.ph = 0.0;
  if (in.swing_state) {  // FootTrajectoryManager::referenceState(leg, phase), trajectory.cpp:360-388
    const SwingState* S = in.swing_state + idx;
    T.has = (int)((stance_word >> (12 + leg)) & 1u);
    // p_start / p_final / the advanced phases may have been written by THIS wave's assembly phase (another lane of it): workgroup
    // scope is all that takes - one wave, one CU, one write-through vector L1, a barrier's release / acquire in between.  Rounds 4-5
    // used agent scope here, which on this multi-die part means "visible across XCDs": every one of the four 8-byte phase stores
    // went out as its own write-through (WRITE_SIZE 1.40x the bytes written: profiles/r06a_tick_full262144) and every load
    // bypassed the L1 that held the line.
#pragma unroll
    for (int r = 0; r < 3; r++) {
      T.a[r] = __hip_atomic_load(&S->p_start[3 * leg + r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      T.b[r] = __hip_atomic_load(&S->p_final[3 * leg + r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    T.ph = in.gait_dt ? __hip_atomic_load(in.gait_phase + 4 * idx + leg, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) : in.gait_phase[4 * idx + leg];
  } else {
#pragma unroll
    for (int r = 0; r < 3; r++) {
      T.a[r] = in.swing_pos[12 * idx + 3 * leg + r];
      T.b[r] = in.swing_vel[12 * idx + 3 * leg + r];
    }
  }
#pragma unroll
  for (int r = 0; r < 3; r++) {
    T.q[r] = qslot ? qslot[(3 * leg + r) * qstride] : in.joint_q[12 * idx + 3 * leg + r];
    T.qdot[r] = in.joint_qdot[12 * idx + 3 * leg + r];
    T.x[r] = in.x[3 * idx + r];
  }
}
// swing leg: reference foot state -> IK -> J^-1 -> joint PD, commander_node.cpp:482-504; independent of the QP's status
QC_DEV void swing_leg_task(CParams& P, const BatchIn& in, const BatchOut& out, const SwingIn& T, const double (&R)[9]) {
  double sp[3], sv[3];
  if (in.swing_state) {
    track_swing(P, T.ph, T.a, T.b, sp, sv);
    if (!T.has) sp[0] = sp[1] = sp[2] = sv[0] = sv[1] = sv[2] = 0.0;  // no trajectory: FootState() (:387)
  } else {
#pragma unroll
    for (int r = 0; r < 3; r++) { sp[r] = T.a[r]; sv[r] = T.b[r]; }
  }
  double pb[3], vb[3], tau[3];
#pragma unroll
  for (int r = 0; r < 3; r++) {
    pb[r] = R[r] * sp[0] + R[3 + r] * sp[1] + R[6 + r] * sp[2] - T.x[r];  // Rwb^T pos - x (sic, :492)
    vb[r] = R[r] * sv[0] + R[3 + r] * sv[1] + R[6 + r] * sv[2];          // Rwb^T vel (:493)
  }
  const LegGeom g = leg_geom(P, T.leg);
  leg_swing_torque(P, g, pb, vb, T.q, T.qdot, tau);
  store_tau(P, out, T.idx, T.leg, tau, true);
}
// Rwb of the robot in `slot`: the wave's LDS rows (RLDS: the one-lane one-fill kernel parked it there) or global memory
template <int SP, bool RLDS>
QC_DEV void task_rwb(const BatchIn& in, const double* __restrict__ Rplanes, int slot, long idx, double (&R)[9]) {
  if constexpr (RLDS) {
#pragma unroll
    for (int k = 0; k < 9; k++) R[k] = Rplanes[k * SP + slot];
  } else {
    const double* Rp = in.Rwb + 9 * idx;
#pragma unroll
    for (int k = 0; k < 9; k++) R[k] = Rp[k];
  }
}

// joint angles of this lane's robot, requested before anything else in the flush (consumed by torque_pass)
struct TorquePre {
  double q[12];
};
// Few robots in the stock of a lane-group kernel (chain-bound batches: four racing lane groups hold FOUR robots): the legs are
// spread over the lanes of the robot's group, as the force stores are - one robot per lane would walk a lane through all
// four legs while 60 lanes idle (measured: +2 us on the 4 096-robot fused tick).
template <int G>
QC_DEV bool torque_by_group(int out_n) { return G > 1 && out_n <= 64 / G; }
// (`Qplanes` != nullptr - QPARK: the joint angles parked by the fill, plane k of slot s at Qplanes[k * SP + s])
template <int SP, int G, bool STR>
QC_DEV void torque_prefetch(const BatchIn& in, const double* __restrict__ sout, int out_n, int lane, TorquePre& T, const double* __restrict__ Qplanes = nullptr) {
  // (defined in every lane and on both paths: an array written to different extents on two paths stays in memory - scratch)
#pragma unroll
  for (int k = 0; k < 12; k++) T.q[k] = 0.0;
  if (torque_by_group<G>(out_n)) {
    constexpr int FPL = 4 / G;
    const int grp = lane_group<G, STR>(lane);
    if (grp < out_n) {
      const long idx = __double_as_longlong(sout[OUT_IDX * SP + grp]);
      const double* qp = in.joint_q + 12 * idx + 3 * FPL * lane_member<G, STR>(lane);
#pragma unroll
      for (int k = 0; k < 3 * FPL; k++) T.q[k] = qp[k];
    }
  } else if (lane < out_n) {
    if (Qplanes) {  // (wave-uniform)
#pragma unroll
      for (int k = 0; k < 12; k++) T.q[k] = Qplanes[k * SP + lane];
    } else {
      const long idx = __double_as_longlong(sout[OUT_IDX * SP + lane]);
      const double* qp = in.joint_q + 12 * idx;
#pragma unroll
      for (int k = 0; k < 12; k++) T.q[k] = qp[k];
    }
  }
}
// the stance-leg torque map of NL legs of the robot in `slot`, from leg0 on (their joint angles in q[0 .. 3 NL))
template <int SP, bool RLDS, int NL, bool RUNTIME_LEG>
QC_DEV void stance_legs(CParams& P, const BatchIn& in, const BatchOut& out, const double* __restrict__ sout, const double* __restrict__ Rplanes, int slot,
                        int leg0, bool have_swing, const double (&q)[12]) {
  const long idx = __double_as_longlong(sout[OUT_IDX * SP + slot]);
  const unsigned long long sw = (unsigned long long)__double_as_longlong(sout[OUT_STAT * SP + slot]);
  const uint32_t stance = (uint32_t)((unsigned long long)__double_as_longlong(sout[OUT_WORD * SP + slot]) >> 32);
  const int st_out = (stance & 0x100u) ? (int)QC_NOT_PD : (int)(uint32_t)sw;
  double R[9];
  task_rwb<SP, RLDS>(in, Rplanes, slot, idx, R);
  // Branch-free over the legs on purpose: a wave of a one-round launch has its SIMD to itself and a leg's three sincos are
  // serial polynomial chains - interleaved they issue back to back, one leg at a time behind a "does any lane need this
  // leg" branch they ran at ~10 cycles per instruction (8.8 k cycles for the four legs, 6.2 k now).
  LegTrig tr[NL];
#pragma unroll
  for (int i = 0; i < NL; i++) {
    const double qa[3] = {q[3 * i], q[3 * i + 1], q[3 * i + 2]};
    tr[i] = leg_trig(qa);
  }
#pragma unroll
  for (int i = 0; i < NL; i++) {
    const int leg = leg0 + i;
    const bool stl = (stance >> leg) & 1u;
    const bool todo = !(have_swing && !stl);  // (a swing leg with swing references belongs to the swing tasks)
    const bool st = stl && st_out == QC_SOLVED;
    double f[3], fb[3], tau[3];
#pragma unroll
    for (int k = 0; k < 3; k++) f[k] = sout[(OUT_F + 3 * leg + k) * SP + slot];
#pragma unroll
    for (int r = 0; r < 3; r++) fb[r] = st ? -(R[r] * f[0] + R[3 + r] * f[1] + R[6 + r] * f[2]) : 0.0;  // BC.cpp:218-232
    if constexpr (RUNTIME_LEG) leg_jt_force(leg_geom(P, leg), tr[i], fb, tau);
    else leg_jt_force(P, i, tr[i], fb, tau);  // (compile-time leg: the constants are scalar operands)
    if (todo) store_tau(P, out, idx, leg, tau, st);
  }
}
template <int SP, bool RLDS, int G, bool STR>
QC_DEV void torque_pass(const DevParams* __restrict__ Pg, const BatchIn& in, const BatchOut& out, const double* __restrict__ sout, int out_n, int lane,
                        const double* __restrict__ Rplanes, TorquePre& Q, const double* __restrict__ Qplanes = nullptr) {
  QC_CLK_ABS(8, 13);
  unsigned char* const tl = reinterpret_cast<unsigned char*>(const_cast<double*>(sout) + OUT_PLANES * SP);  // (TASK_DOUBLES behind the planes)
  const bool have_swing = in.swing_pos || in.swing_state;
  const bool mine = lane < out_n;
  uint32_t stance = 0xFu;
  if (mine) stance = (uint32_t)((unsigned long long)__double_as_longlong(sout[OUT_WORD * SP + lane]) >> 32);
  // the swing-leg tasks of the wave, leg-major (neighbouring lanes touch neighbouring robots): one byte each, slot << 2 | leg
  int ns = 0;
  if (have_swing) {
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const bool sw = mine && !((stance >> i) & 1u);
      const unsigned long long ms = __builtin_amdgcn_ballot_w64(sw);
      if (sw) tl[ns + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(ms >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)ms, 0))] = (unsigned char)((lane << 2) | i);
      ns += __builtin_popcountll(ms);
    }
    __syncthreads();
  }
  // The joint angles requested at the top of the flush have to BE here before the swing inputs are requested: vector-memory
  // results return in order, so waiting for them later would wait for the (slower, L1-bypassing) swing loads as well.
#pragma unroll
  for (int k = 0; k < 12; k++) asm volatile("" : "+v"(Q.q[k]));
  SwingIn nxt;
  int nslot = 0;
  if (lane < ns) {  // the first swing pass's inputs: in flight while the stance legs are computed
    const int code = tl[lane];
    nslot = code >> 2;
    swing_fetch(in, __double_as_longlong(sout[OUT_IDX * SP + nslot]), code & 3,
                (uint32_t)((unsigned long long)__double_as_longlong(sout[OUT_WORD * SP + nslot]) >> 32), nxt, Qplanes ? Qplanes + nslot : nullptr, SP);
  }
  asm volatile("" ::: "memory");  // (... and requested above this line, not behind the stance legs' arithmetic)
  QC_CLK_ABS(13, 15);
  // stance legs (and the swing legs of a batch without swing references: zero torque), one robot per lane - or, with few
  // robots in a lane-group kernel, the legs of a robot spread over its group: tau = clamp(J^T f_body), kinematics.cpp:219-231,
  // commander_node.cpp:511-526
  {
    CParams& P = *QC_PARAMS_HERE(Pg);
    if (torque_by_group<G>(out_n)) {
      if constexpr (G > 1) {
        const int grp = lane_group<G, STR>(lane);
        if (grp < out_n) stance_legs<SP, RLDS, 4 / G, true>(P, in, out, sout, Rplanes, grp, (4 / G) * lane_member<G, STR>(lane), have_swing, Q.q);
      }
    } else if (mine) {
      stance_legs<SP, RLDS, 4, false>(P, in, out, sout, Rplanes, lane, 0, have_swing, Q.q);
    }
  }
  QC_CLK_ABS(15, 14);
#pragma unroll 1
  for (int t = lane; t < ns; t += 64) {
    const SwingIn cur = nxt;
    const int cslot = nslot;
    if (t + 64 < ns) {  // the next pass's inputs are requested before this pass computes
      const int code = tl[t + 64];
      nslot = code >> 2;
      swing_fetch(in, __double_as_longlong(sout[OUT_IDX * SP + nslot]), code & 3,
                  (uint32_t)((unsigned long long)__double_as_longlong(sout[OUT_WORD * SP + nslot]) >> 32), nxt, Qplanes ? Qplanes + nslot : nullptr, SP);
    }
    double R[9];
    task_rwb<SP, RLDS>(in, Rplanes, cslot, cur.idx, R);
    swing_leg_task(*QC_PARAMS_HERE(Pg), in, out, cur, R);
  }
  QC_CLK_ABS(14, 8);
}

// store the robots parked in the output stock: one per lane, or one per lane group when there are few
template <int G, bool KIN, bool STR, int SP, bool RLDS = false>
QC_DEV void flush_out(const DevParams* __restrict__ Pg, const BatchIn& in, const BatchOut& out, const double* __restrict__ sout, int out_n, int lane,
                      const double* __restrict__ Rplanes = nullptr, const double* __restrict__ Qplanes = nullptr) {
  TorquePre tq;
  if constexpr (KIN) {
    if (out.joint_tau) {
      torque_prefetch<SP, G, STR>(in, sout, out_n, lane, tq, Qplanes);
      asm volatile("" ::: "memory");  // (requested HERE: left alone, the compiler sinks these loads to their first use, behind the swing inputs)
    }
  }
  if (G > 1 && out_n <= 64 / G) {
    const int grp = lane_group<G, STR>(lane);
    if (grp < out_n) {
      CParams& P = *QC_PARAMS_HERE(Pg);
      store_from_stock<KIN, 4 / G, SP>(P, in, out, sout, grp, lane_member<G, STR>(lane));
    }
  } else if (lane < out_n) {
    CParams& P = *QC_PARAMS_HERE(Pg);
    store_from_stock<KIN, 4, SP, RLDS>(P, in, out, sout, lane, 0, RLDS ? Rplanes + lane : nullptr);
  }
  if constexpr (KIN) {
    if (out.joint_tau) torque_pass<SP, RLDS, G, STR>(Pg, in, out, sout, out_n, lane, Rplanes, tq, Qplanes);
  }
}

// record of one running robot in the re-pack area (37 doubles: odd, so the four lanes of a group read different
// banks): 0-5 b, 6 idx, 7 {iters, output slot, stance}, 8-19 r, 20-31 f, 32-35 face code per foot
constexpr int REPACK_RS = 37;
template <class LaneX>
QC_DEV void repack_write(const LaneX& L, double* __restrict__ rec, int slot, int member) {
  constexpr int FPL = LaneX::FPL;
  if (member == 0) {
#pragma unroll
    for (int k = 0; k < 6; k++) rec[k] = L.Wr.b[k];
    rec[6] = __longlong_as_double(L.idx);
    rec[7] = __longlong_as_double((long long)(((unsigned long long)(uint32_t)((L.iters << 8) | slot) << 32) | L.stance | L.polish_bit()));
  }
#pragma unroll
  for (int i = 0; i < FPL; i++) {
    const int ft = L.foot0 + i;
#pragma unroll
    for (int k = 0; k < 3; k++) {
      rec[8 + 3 * ft + k] = L.Wr.r[i][k];
      rec[20 + 3 * ft + k] = L.f[3 * i + k];
    }
    rec[32 + ft] = __longlong_as_double((long long)L.foot_code(i));
  }
}
// ... and into member j4 of a 4-lane group; returns the robot's slot in the output stock
template <class Lane4X, class Eqp4X>
QC_DEV int repack_read(const DevParams* __restrict__ Pg, Lane4X& L4, Eqp4X& eqp4, const double* __restrict__ rec, int j4) {
#pragma unroll
  for (int k = 0; k < 6; k++) {
    L4.Wr.b[k] = rec[k];  // (already -b: both sides are 6x6 forms)
    asm volatile("" : "+v"(L4.Wr.b[k]));
  }
#pragma unroll
  for (int k = 0; k < 3; k++) {
    L4.Wr.r[0][k] = rec[8 + 3 * j4 + k];
    L4.f[k] = rec[20 + 3 * j4 + k];
  }
  const uint32_t fw = (uint32_t)__double_as_longlong(rec[32 + j4]);
  L4.idx = __double_as_longlong(rec[6]);
  const unsigned long long fl = (unsigned long long)__double_as_longlong(rec[7]);
  L4.stance = (uint32_t)fl & ~QC_POLISH_ONE;
  L4.iters = (int)(fl >> 40);
  L4.foot0 = j4;
  L4.set_foot_code(0, fw);
  if constexpr (Lane4X::kArith) L4.set_face_const(*QC_PARAMS_HERE(Pg));
  L4.status = QC_MAX_ITER;
  {
    const double tol = Lane4X::kTol * QC_PARAMS_HERE(Pg)->tol_d;
    L4.tol_s = ((uint32_t)fl & QC_POLISH_ONE) ? tol : -tol;
  }
  L4.have_f = true;
  eqp4.setup(*QC_PARAMS_HERE(Pg), L4.Wr, j4);
  return (int)((fl >> 32) & 0xFFu);
}

// One or two lanes per robot: once at most 16 robots of a wave are still running they fit a 4-lanes-per-robot layout,
// whose recalculation is much shorter (487 instructions against 730 at two lanes and ~1170 at one) - and the wave
// waits for exactly these stragglers.  The running robots are re-packed through the (now idle) input stock and finish
// on the G = 4 body; `slot` is where the robot's result goes in the output stock.  `bm` = ballot(busy), at most
// 16 robots.
// Two stages (strided layout): while more than 8 robots run, the classic body.  Then the survivors are re-packed once
// more, each into TWO groups 8 lanes apart that continue with different drop rules - most negative multiplier / all
// negative multipliers - and the first at the KKT point wins (the racing strategies of the mode-2 kernel, applied to
// the robots every other lane of the wave is waiting for).  Forking after ~6 recalculations still shortens the
// slowest robot's chain: 20 -> 16 on config 3's 16 384 first robots, mean of the per-wave maximum 11.5 -> 10.6
// (oracle/prototypes/proto_tail_fork.py); clamp-step variants add nothing at that point.
// HOLD (the joint_q one-lane kernel, whose re-pack records ALIAS the output stock - see QPARK in balance_kernel): no result is parked
// before the last read of a record; the classic stage's finishers keep theirs in registers (three doubles and a few words per lane) until
// the race stage is over.
template <bool KIN, bool UNIFORM, int SP, bool HOLD = false, class LaneG>
QC_DEV void finish_on_four_lanes(const DevParams* __restrict__ Pg, const LaneG& L, bool busy, unsigned long long bm, int slot, int member, int lane,
                                 double* __restrict__ sin, double* __restrict__ sout, const bool cold) {
  using Eqp4 = EqpDiagW<UNIFORM, 4>;
  using Lane4 = Lane<Eqp4, KIN>;
  using LaneR = Lane<Eqp4, KIN, true>;  // with a per-lane drop rule
  constexpr int GS = LaneG::G;  // lanes per robot of the layout being left
  constexpr int RS = REPACK_RS;
  const int nb = __builtin_popcountll(bm) / GS;  // running robots
  if (nb == 0) return;
  QC_CLK_TAIL_BEGIN();
  static_assert(16 * RS <= (HOLD ? OUT_PLANES : IN_PLANES) * SP, "the re-pack records live in the idle input stock (HOLD: under the output stock)");
  const int rank2 = __builtin_amdgcn_mbcnt_hi((unsigned)(bm >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bm, 0)) / GS;
  __syncthreads();  // nobody reads the input stock any more
  if (busy) repack_write(L, sin + rank2 * RS, slot, member);
  __syncthreads();
  const int g4 = lane_group<4, true>(lane), j4 = lane_member<4, true>(lane);
  // (a warm-started robot that is not done after its first recalculation is a face or two away: nothing to race for;
  // measured neutral to +0.5 us on config 4's tick, tools/tail_race_scan.py)
  const bool race = cold && QC_PARAMS_HERE(Pg)->tail_race != 0;
  int nrun = nb;  // robots the race stage starts with (the first re-pack's records if the classic stage is skipped)
  QC_CLK_TAIL_LOOP();
  Lane4 L4;
  bool held = false;  // HOLD: this group's classic-stage result is still in L4
  int slot_held = 0;
  if (!race || nb > 8) {
    Eqp4 eqp4(nullptr);
    bool busy4 = g4 < nb;
    // groups beyond the running robots shadow record 0: the strided layout keeps every lane in the loop (MFMA)
    const int slot4 = repack_read(Pg, L4, eqp4, sin + (busy4 ? g4 : 0) * RS, j4);
    const int stop = race ? 8 : 0;
    // the tail has the registers to keep the recalculation's constants resident, as the mode-2 kernel does
    Recalc<UNIFORM> rc(Pg);
    while (__builtin_popcountll(__builtin_amdgcn_ballot_w64(busy4) & 0xFFFFull) > stop) {
      QC_CLK(7, 2);
      const bool done = rc.template step<Lane4::STEADY>(L4, eqp4, busy4);
      busy4 = busy4 & !done;
    }
    if constexpr (HOLD) {
      held = g4 < nb && !busy4;
      slot_held = slot4;
    } else {
      if (g4 < nb && !busy4) L4.template push_result<SP>(sout, slot4);
    }
    const unsigned run16 = (unsigned)(__builtin_amdgcn_ballot_w64(busy4) & 0xFFFFull);  // (member 0 of the strided groups = lanes 0-15)
    nrun = __builtin_popcount(run16);
    if (nrun == 0) {
      if constexpr (HOLD) {
        __syncthreads();  // every record has been read
        if (held) L4.template push_result<SP>(sout, slot_held);
      }
      QC_CLK_TAIL_END();
      return;
    }
    // second re-pack: the <= 8 survivors
    const int rank = __builtin_popcount(run16 & ((1u << g4) - 1u));
    __syncthreads();
    if (busy4) repack_write(L4, sin + rank * RS, slot4, j4);
    __syncthreads();
  }
  LaneR LR;
  Eqp4 eqpR(nullptr);
  const int r = g4 & 7, sid = g4 >> 3;  // robot, strategy of this group
  bool busyR = r < nrun;
  const int slotR = repack_read(Pg, LR, eqpR, sin + (busyR ? r : 0) * RS, j4);
  LR.drop_all = sid == 1;
  unsigned solved_mask = 0;  // strategies of this lane's robot that have reached the KKT point
  auto after = [&](bool done) {
    const int mine = (busyR & LR.kkt) ? (1 << sid) : 0;
    const int m = race_or<8, 2>(mine);
    solved_mask |= (unsigned)m;
    busyR = busyR & !done & (solved_mask == 0);
  };
  Recalc<UNIFORM> rcR(Pg);
  while (__builtin_amdgcn_ballot_w64(busyR) != 0) {
    QC_CLK(7, 2);
    after(rcR.template step<LaneR::STEADY>(LR, eqpR, busyR));
  }
  QC_CLK_TAIL_END();
  // the winner - the lower-numbered strategy if both got there in the same recalculation, strategy 0 with whatever
  // status it has if none did - parks the result
  const int win = solved_mask ? __builtin_ctz(solved_mask) : 0;
  if constexpr (HOLD) __syncthreads();  // (the race stage's records have been read by every group)
  if (r < nrun && sid == win) LR.template push_result<SP>(sout, slotR);
  if constexpr (HOLD) {
    if (held) L4.template push_result<SP>(sout, slot_held);
  }
}

// How many of a cold-started robot's first recalculations are CLAMP steps (project the equality-constrained minimiser
// of the current working set into the frusta, keep the faces it hits) before the ratio-test steps start.  One is the
// classic start.  More of them build the working set several faces at a time and cost less than a ratio-test step:
// five are the measured optimum where the batch fills the chip (one or two lanes per robot: 262 144 robots 104 -> 95 us,
// 1 M robots 345 -> 291 us; more than six start to cycle - profiles/r02_clamp_scan.log); the 4-lane kernels (chain-bound
// batches) do not care, and a warm-started robot already has its working set: further clamp steps only disturb it.
template <int G>
QC_DEV int clamp_steps_for(CParams& P, const uint32_t* warm) {
  const int tuned = P.clamp_steps;  // qc_set_tuning "clamp_steps"; 0 = this rule
  return tuned > 0 ? tuned : ((warm != nullptr || G == 4) ? 1 : 5);
}

// MODE 1: the launch gives every wave one fill (chunk <= 64 / G).  MODE 2: one fill and the SIMD to itself,
// recalculation constants resident in VGPRs.
// RACE (strided 4-lane one-fill kernels): strategies racing per robot, 1, 2 or 4; a wave then holds 16 / RACE robots (see Lane).

// The dynamic LDS of one balance_kernel instantiation: what the kernel addresses and what the launch asks for (offsets in doubles
// from the start of the workgroup's LDS).
template <class Eqp, bool KIN, int MODE>
struct LdsLayout {
  static constexpr int G = Eqp::G;
  static constexpr int SP = stock_slots(G) + 1;  // plane stride of the stock
  // One-lane dense form as one-fill workgroups (round 5): the 78 Hessian planes (39 936 B) ARE the workgroup's LDS - four
  // workgroups per CU, one per SIMD.  With the stock in front of them (58.3 KB) a CU held two, i.e. every other SIMD idled
  // behind the 512-register kernel.  The input stock is not used on this path (one lane assembles and solves its robot),
  // Rwb is read again for the output transform instead of parked, and the output stock aliases the first Hessian planes
  // once every robot of the wave is finished.
  static constexpr bool HESS_ONLY = Eqp::kHessianInLds;
  static_assert(!HESS_ONLY || (OUT_PLANES * SP + TASK_DOUBLES <= Eqp::kLdsDoubles), "the output stock fits the Hessian planes it aliases");
  // (see QPARK_* above: Rwb and the joint angles parked, the re-pack records under the output stock)
  static constexpr bool QPARK = KIN && G == 1 && MODE == 1 && !HESS_ONLY;
  static_assert(!QPARK || SP == 65, "the QPARK layout is laid out for 64 slots");
  // One lane per robot: Rwb is parked in the first nine planes of the (otherwise idle) input-stock area for the output transform;
  // the planes behind them serve as the re-pack area of the tail.
  static constexpr bool RPARK = G == 1 && !HESS_ONLY;
  static constexpr int R_PLANES = RPARK ? 9 : 0;
  static constexpr int IN = 0;                                                            // input stock (one lane per robot: Rwb planes)
  static constexpr int OUT = HESS_ONLY ? 0 : (QPARK ? QPARK_OUT : IN_PLANES) * SP;        // output stock
  static constexpr int REPACK = QPARK ? OUT : R_PLANES * SP;                              // re-pack records of the 4-lane tail
  static_assert(G != 1 || QPARK || (R_PLANES * SP + 16 * REPACK_RS <= IN_PLANES * SP), "Rwb planes + re-pack records fit the input-stock area");
  static constexpr int EQP = HESS_ONLY ? 0 : stock_doubles(stock_slots(G));               // the form's own planes (Eqp::kLdsDoubles of them)
  static constexpr size_t BYTES = sizeof(double) * (HESS_ONLY ? (size_t)Eqp::kLdsDoubles
                                                    : QPARK   ? (size_t)qpark_doubles()
                                                              : (size_t)(EQP + Eqp::kLdsDoubles));
};

// The kernel's argument block as the launch lays it out (kernarg segment), for re-deriving BatchIn / BatchOut AT THEIR USE in the
// joint_q kernels: 23 array pointers held in SGPRs from the kernel's entry to its flush - across a solve that needs none of
// them - do not fit the 102-SGPR file next to the loop's masks, and the compiler parks them in VGPR lanes (108-175 spilled
// SGPRs, ~250 v_readlane per wave: profiles/r05_kernel_resources.txt).  Read again from the (constant, scalar-cached) kernarg
// segment where they are used, behind an opaque pointer so that they are not kept live in between, they cost a few s_loads.
struct BalanceKernelArgs {
  const DevParams* Pg;
  long n;
  BatchIn in;
  const uint32_t* warm;
  BatchOut out;
  long chunk;
};
template <class T>
QC_DEV const T& kernarg_here(unsigned off) {
  const __attribute__((address_space(4))) char* p = (const __attribute__((address_space(4))) char*)__builtin_amdgcn_kernarg_segment_ptr();
  p += off;
  asm volatile("" : "+s"(p));
  return *(const T*)(const __attribute__((address_space(4))) T*)p;
}

template <class Eqp, bool KIN, int MIN_WAVES_PER_SIMD, int MODE, int RACE = 1>
__global__ __launch_bounds__(64, MIN_WAVES_PER_SIMD) void balance_kernel(const DevParams* __restrict__ Pg, const long n, const BatchIn in_k,
                                                                         const uint32_t* __restrict__ warm, const BatchOut out_k, const long chunk) {
  static_assert(MODE == 1 || MODE == 2, "one fill per wave (MODE 1), and the SIMD to itself (MODE 2)");
  static_assert(RACE == 1 || (Eqp::kStrided && Eqp::G == 4), "racing strategies exist for the strided 4-lane kernels");
  constexpr int G = Eqp::G;
  // (KIN: re-read from the kernarg segment at every use, see BalanceKernelArgs; the QP-only kernels hold 14 pointers and keep them,
  // and so does the one-wave-per-SIMD kernel of chain-bound batches - a lone wave waits out every scalar-load round trip: the fused
  // tick on 4 096 robots 27.36 -> 27.55 us with it, profiles/r06_tick_ab.log)
  constexpr bool REREAD = KIN && MODE != 2;
  auto IN = [&]() -> const BatchIn& {
    if constexpr (REREAD) return kernarg_here<BatchIn>((unsigned)offsetof(BalanceKernelArgs, in));
    else return in_k;
  };
  auto OUT = [&]() -> const BatchOut& {
    if constexpr (REREAD) return kernarg_here<BatchOut>((unsigned)offsetof(BalanceKernelArgs, out));
    else return out_k;
  };
  extern __shared__ __attribute__((aligned(16))) double qc_lds[];  // [stock planes][64] (+ the dense form's 78 Hessian planes)
  using Lay = LdsLayout<Eqp, KIN, MODE>;
  constexpr int SP = Lay::SP;
  constexpr bool HESS_ONLY = Lay::HESS_ONLY, QPARK = Lay::QPARK;
  double* const sin = qc_lds + Lay::IN;
  double* const sout = qc_lds + Lay::OUT;
  // XCD-aware workgroup -> chunk map.  The dispatcher places workgroup b on XCD b % 8 (observed, MI355X_MICROARCH.md "Workgroup
  // dispatch"; a speed assumption only - any placement computes the same robots), each XCD with an L2 of its own.  A racing wave holds
  // 4 (or 8) robots: 288 contiguous bytes per 72-byte-row array, so neighbouring waves share the 128-byte lines their rows straddle,
  // and with the identity map - neighbours on different XCDs - every shared line is fetched from HBM once per XCD: 1.6x the algorithmic
  // bytes on config 2 (profiles/r02 ... r04_cfg2).  Sixteen robots are line-aligned in every array (16 x 72 B = 9 lines), so the waves
  // of one aligned 16-robot group are mapped to ONE XCD and the groups go round the XCDs as before.  (Mapping whole contiguous eighths of
  // the batch to an XCD removes the same re-fetches but costs config 2 0.2 us, profiles/r05_ab_xcd_map.log: the spreading of
  // neighbouring groups over the XCDs is worth keeping.)  Waves of 16 robots or more share no line: identity.
  unsigned chunk_id = blockIdx.x;
  if constexpr (RACE > 1) {  // 16 / RACE robots per wave: RACE waves per aligned group (compile-time powers of two: shifts and masks only -
    // with run-time divisions the map cost the wave's first 0.1 us more than it saved)
    constexpr unsigned gw = (unsigned)RACE, super = 8u * gw;
    const unsigned full = gridDim.x & ~(super - 1u);
    if (blockIdx.x < full && chunk == 16 / RACE) {
      const unsigned xcd = blockIdx.x & 7u, slot = blockIdx.x >> 3;
      chunk_id = (slot / gw) * super + xcd * gw + (slot % gw);
    }
  }
  long cursor = (long)chunk_id * chunk;  // wave-uniform: next robot of this wave's chunk to assemble
  const long end = cursor + chunk < n ? cursor + chunk : n;
  const int lane = threadIdx.x;
  constexpr bool STR = Eqp::kStrided;  // lane layout of a group
  const int member = lane_member<G, STR>(lane);
  int stock_n = 0;  // input stock: slots [0, stock_n) hold assembled robots
  // one-lane dense form, QP only: stragglers fork into idle lanes with the other drop rule.  (Not the joint_q kernel: with the results
  // parked in the lanes' own dead Hessian columns for the torque pass - tools/experiments/r06_dense_kin_twin.patch - the race bought its
  // tick nothing, 151.4 us with it, 151.4 with race = 0, 147.8 without the machinery: profiles/r06_dense_tick.log.  That kernel's time
  // is its fill and flush at one wave per SIMD, not its stragglers.)
  constexpr bool TWIN = Eqp::kHessianInLds && !KIN;
  Lane<Eqp, KIN, (RACE > 1) || TWIN> L;
  L.idx = -1;
  L.foot0 = member * (4 / G);
  Eqp eqp(qc_lds + Lay::EQP + lane);
  bool busy = false;  // group holds an unfinished robot
  QC_CLK_BEGIN();
  // One fill per wave, a divergent solve loop, one push, one flush: nothing but recalculations on the serial chain that
  // bounds such a batch.
  constexpr bool RESIDENT = MODE == 2;
  if (cursor >= end) return;
  UConst uc;  // RESIDENT: the recalculation's constants live in VGPRs (no scalar load + wait per recalculation)
  if constexpr (RESIDENT) uc = load_uconst(*QC_PARAMS_HERE(Pg));
  // One lane per robot: the lane that assembles a robot is the lane that solves it, so the robot goes straight from the
  // assembly into the solver's registers - no input stock, no barrier - and its Rwb is parked in LDS for the output transform
  // (LdsLayout::RPARK).
  constexpr bool DIRECT = G == 1;
  constexpr bool RPARK = Lay::RPARK;
  if constexpr (DIRECT) {
    const long left = end - cursor;
    stock_n = left < 64 ? (int)left : 64;
    if (lane < stock_n) {
      // Everything the fill reads from memory is issued back to back - the contact bytes and the warm-start word first
      // (behind wave-uniform null tests), then the 48 doubles of the state - and nothing dependent sits in between: a
      // wave's fill used to chain four to five vector-memory round trips (two batches of state, contact bytes, warm word,
      // Rwb again: 2.5 us from kernel entry to "inputs landed" for a lone wave, profiles/r03_timeline.log).
      const BatchIn& ia = IN();
      const uint32_t* wp = warm;
      const long robot = cursor + lane;
      const uint32_t sw = ia.stance ? *reinterpret_cast<const uint32_t*>(ia.stance + 4 * robot) : 0u;
      const uint32_t wv = wp ? wp[robot] : 0u;
      RawState S;
      TickExtra X;
      double fp[12];
      fetch_extra<KIN>(ia, robot, X);
      fetch_state<4, KIN>(ia, robot, 0, S, fp);
      asm volatile("" ::: "memory");  // (the loads above stay above)
      CParams& P = *QC_PARAMS_HERE(Pg);
      Wrench<4> W;
      const uint32_t st = assemble_from_state<KIN, 4, false>(P, ia, robot, 0, S, fp, sw, X, W);
      if constexpr (RPARK) {
#pragma unroll
        for (int k = 0; k < 9; k++) sin[k * SP + lane] = S.R[k];
      }
      if constexpr (QPARK) {  // (fp = the twelve joint angles fetch_state read)
#pragma unroll
        for (int k = 0; k < 12; k++) sin[(QPARK_Q + k) * SP + lane] = fp[k];
      }
      L.load_direct(W, st, wv, robot, 0, P.tol_start);
    } else if constexpr (TWIN) {
      // The wave-uniform loops below run every lane through the recalculation body, the lanes beyond a ragged last fill
      // included: they carry a defined robot - no wrench, no stance foot (every foot eliminated, nothing to iterate on) -
      // instead of whatever the registers held.  They never store.  (Shadowing robot 0 of the wave, as the strided kernels'
      // spare groups do, costs this 512-register kernel 12 B of scratch.)
      Wrench<4> W;
#pragma unroll
      for (int k = 0; k < 6; k++) W.b[k] = 0.0;
#pragma unroll
      for (int i = 0; i < 4; i++) W.r[i][0] = W.r[i][1] = W.r[i][2] = 0.0;
      L.load_direct(W, 0u, 0u, -1, 0, 0.0);
    }
  } else {
    stock_n = restock<G, KIN, STR, SP>(Pg, IN(), warm, cursor, end, lane, member, sin);
  }
  const int grp = lane_group<G, STR>(lane);
  busy = grp < stock_n;
  // measurement probe (qc_set_tuning "probe_batch_load"): load -> assemble -> store only, no recalculation
  const bool probe = QC_PARAMS_HERE(Pg)->max_iter == 0;
  using LaneT = Lane<Eqp, KIN, (RACE > 1) || TWIN>;
  if constexpr (STR) {
    // Strided layout: the group sums run on the matrix pipe, and an MFMA reads its operands from ALL 64 lanes
    // whatever EXEC says - the all-ones A operand included, which the compiler materialises under the current
    // EXEC.  So nothing here may run under a partial EXEC: every lane carries a robot (groups beyond the fill
    // shadow robot 0) through a wave-uniform loop, and only the lanes of running robots commit what a
    // recalculation produced.
    // RACE > 1: the wave holds 16 / RACE robots; group grp solves robot grp % ROB with strategy sid
    constexpr int ROB = 16 / RACE;
    const int slot = grp & (ROB - 1);
    const int sid = (grp / ROB) * (4 / RACE);  // 4 strategies: 0 .. 3; 2: {0, 2}
    if constexpr (RACE > 1) {
      busy = slot < stock_n;
      // (clamp steps, drop rule) = (1, most negative) (1, all) (2, all) (3, most negative): over eight 4 096-robot
      // batches the slowest robot takes 13.25 recalculations on average against 16.9 with the first strategy alone
      // (13.9 for the pair {0, 2} a 2-way race runs); oracle/prototypes/proto_race_strategies.py
      L.nclamp = sid == 3 ? 3 : (sid == 2 ? 2 : 1);
      L.drop_all = sid == 1 || sid == 2;
    }
    double tol0;  // (RESIDENT: from the register copy - another scalar load here is a memory round trip a lone wave waits out)
    if constexpr (RESIDENT) tol0 = uc.tol_start;
    else tol0 = QC_PARAMS_HERE(Pg)->tol_start;
    L.template load_from_stock<SP>(sin, busy ? slot : 0, member, tol0);
    if constexpr (LaneT::kArith) {  // (guarded here: deriving the constants' pointer costs the other forms a scalar move)
      if constexpr (RESIDENT) L.set_face_const(uc);
      else L.set_face_const(*QC_PARAMS_HERE(Pg));
    }
    eqp.setup(*QC_PARAMS_HERE(Pg), L.Wr, L.foot0);
    busy = busy && !probe;
    unsigned solved_mask = 0;  // RACE: strategies of this lane's robot that have reached the KKT point
    // The lanes whose robot is still running, as the wave's lane mask (a scalar pair).  The loops below test it as the integer it
    // is, and a recalculation takes its `live` from it for nothing (a lane mask is what a select reads).  Carried as a per-lane
    // bool instead, `busy` went through a VGPR byte: written and compared after every recalculation for the ballot, masked and
    // compared twice at the top of the next - and a loop whose test is a ballot (a convergent operation, which loop rotation does
    // not duplicate) stays top-tested, so everything live past it (f, status and count, the working-set word, the race's mask)
    // was copied at the header of every recalculation and the exit was a block of its own with mask merges at the latch.
    // Racing kernels of the packed lanes (the 6x6 uniform form) only.  The 4-lane kernels without a race keep the per-lane flag:
    // with the mask the uniform form's mode-2 kernel needs ten registers more and loses its third wave per SIMD.  So do the
    // general and the dense form's racing kernels, which it costs 16 VGPRs and eight more registers parked in AGPRs.
    constexpr bool MASKED = RACE > 1 && LaneT::kWord;
    unsigned long long running = MASKED ? __builtin_amdgcn_ballot_w64(busy) : 0ull;
    auto any_running = [&]() {
      if constexpr (MASKED) return running != 0;
      else return __builtin_amdgcn_ballot_w64(busy) != 0;
    };
    auto live_now = [&]() -> bool {
      if constexpr (MASKED) return __builtin_amdgcn_inverse_ballot_w64(running);
      else return busy;
    };
    // the robot is finished as soon as one strategy has solved it; the others stop with it
    auto after = [&](bool live, bool done) {
      if constexpr (RACE > 1 && !MASKED) {
        const int mine = (busy & L.kkt) ? (1 << sid) : 0;
        const int m = race_or<ROB, RACE>(mine);
        solved_mask |= (unsigned)m;
        busy = busy & !done & (solved_mask == 0);
      } else if constexpr (RACE > 1) {
        const int mine = L.kkt ? (1 << sid) : 0;  // (kkt = live & solved: Lane::iterate)
        const int m = race_or<ROB, RACE>(mine);
        solved_mask |= (unsigned)m;
        // live & !done & (solved_mask == 0) as ONE compare: what stops the robot, any non-zero value for a lane that stops by itself
        unsigned stop = (live & !done) ? solved_mask : 1u;
        asm volatile("" : "+v"(stop));  // (opaque: folded back into the three conditions it is a compare, a mask AND, a select and a second compare)
        running = __builtin_amdgcn_ballot_w64(stop == 0u);
      } else {
        busy = busy & !done;
      }
    };
    QC_CLK(0, 2);
    // clamp steps: one for the racing lanes (their strategies take more in the MIXED recalculations below)
    const int first_steps = RACE > 1 ? 1 : clamp_steps_for<G>(*QC_PARAMS_HERE(Pg), warm);
#pragma unroll 1
    for (int k = 0; k < first_steps && (k == 0 || any_running()); k++) {
      if (k) QC_CLK(7, 2);
      const bool live = live_now();
      bool done;
      if constexpr (RESIDENT) {
        pin_uconst(uc);
        done = L.template iterate<LaneT::FIRST>(uc, eqp, live, k == 0 && warm == nullptr);
      } else {
        done = L.template iterate<LaneT::FIRST>(*QC_PARAMS_HERE(Pg), eqp, live, k == 0 && warm == nullptr);
      }
      after(live, done);
    }
    if constexpr (RACE > 1) {  // recalculations 2 and 3: clamp steps for the strategies that take them, ordinary steps for the others
#pragma unroll 1
      for (int it = 2; it <= 3 && any_running(); it++) {
        QC_CLK(7, 2);
        const bool live = live_now();
        bool done;
        if constexpr (RESIDENT) {
          pin_uconst(uc);
          done = L.template iterate<LaneT::MIXED>(uc, eqp, live);
        } else {
          done = L.template iterate<LaneT::MIXED>(*QC_PARAMS_HERE(Pg), eqp, live);
        }
        after(live, done);
      }
    }
    while (any_running()) {
      QC_CLK(7, 2);
      const bool live = live_now();
      bool done;
      if constexpr (RESIDENT) {
        pin_uconst(uc);
        done = L.template iterate<LaneT::STEADY>(uc, eqp, live);
      } else {
        done = L.template iterate<LaneT::STEADY>(*QC_PARAMS_HERE(Pg), eqp, live);
      }
      after(live, done);
    }
    // RACE: the winner - the lowest-numbered strategy among those that solved the robot in the deciding
    // recalculation, or strategy 0 with whatever status it has if none did - parks the result (no race: slot = grp)
    const int win = (RACE > 1 && solved_mask) ? __builtin_ctz(solved_mask) : 0;
    QC_CLK(7, 8);
    if (slot < stock_n && (RACE == 1 || sid == win)) L.template push_result<SP>(sout, slot);
    __syncthreads();
    flush_out<Eqp::G, KIN, STR, SP>(Pg, IN(), OUT(), sout, stock_n, lane);
    QC_CLK_END(8);
    return;
  }
  if (busy || TWIN) {  // (TWIN: the shadow lanes of a ragged fill get their Hessian column too)
    if constexpr (!DIRECT) L.template load_from_stock<SP>(sin, grp, member, QC_PARAMS_HERE(Pg)->tol_start);
    eqp.setup(*QC_PARAMS_HERE(Pg), L.Wr, L.foot0);
  }
  const bool mine = busy;
  busy = busy && !probe;
  QC_CLK(0, 2);
  const int first_steps = clamp_steps_for<G>(*QC_PARAMS_HERE(Pg), warm);
#pragma unroll 1
  for (int k = 0; k < first_steps; k++) {
    if (k) QC_CLK(7, 2);
    if (busy) {  // every robot of a one-fill wave is fresh exactly once: the clamp steps are peeled
      if constexpr (RESIDENT) {
        pin_uconst(uc);
        busy = !L.template iterate<LaneT::FIRST>(uc, eqp, true, k == 0 && warm == nullptr);
      } else {
        busy = !L.template iterate<LaneT::FIRST>(*QC_PARAMS_HERE(Pg), eqp, true, k == 0 && warm == nullptr);
      }
    }
  }
  if constexpr (Eqp::kRepackTail) {
    unsigned long long bm = __builtin_amdgcn_ballot_w64(busy);
    while (__builtin_popcountll(bm) > 16 * G) {  // more than 16 robots still running
      QC_CLK(7, 2);
      if (busy) busy = !L.template iterate<LaneT::STEADY>(*QC_PARAMS_HERE(Pg), eqp);
      bm = __builtin_amdgcn_ballot_w64(busy);
    }
    if constexpr (QPARK) {
      // the re-pack records live under the output stock: the tail parks its results after its last record read, and the robots that
      // finished on the one-lane body after the tail (their results wait in this lane's registers)
      finish_on_four_lanes<KIN, Eqp::kUniform, SP, true>(Pg, L, busy, bm, grp, member, lane, qc_lds + Lay::REPACK, sout, warm == nullptr);
      if (!busy && mine) L.template push_result<SP>(sout, grp);
    } else {
      if (!busy && mine) L.template push_result<SP>(sout, grp);  // finished in the one- / two-lane layout
      finish_on_four_lanes<KIN, Eqp::kUniform, SP>(Pg, L, busy, bm, grp, member, lane, qc_lds + Lay::REPACK, sout, warm == nullptr);
    }
  } else if constexpr (TWIN) {
    // The one-lane dense form has no 4-lane tail (the exchange tile of the 4-lane dense body does not fit next to the Hessian
    // planes), so a wave walks its one-lane body until its slowest robot is done - at half the lanes or fewer busy for most of
    // that walk.  Those idle lanes race: once at most 32 robots still run, every running robot is copied into an idle lane
    // (working set, point, c; the 78 Hessian entries are READ from the owner's LDS column by both - nobody writes them after
    // setup) which continues with the OTHER drop rule - all negative multipliers at once instead of the most negative one -
    // and whoever reaches the KKT point first ends both (the tail race of the 6x6 forms, profiles/r02_tail_race_scan.log, with
    // lanes instead of lane groups).  Cold batches only: a warm-started robot that is not done after its first recalculation
    // is a face or two away.
    unsigned long long bm = __builtin_amdgcn_ballot_w64(busy);
    const bool fork_ok = warm == nullptr && QC_PARAMS_HERE(Pg)->tail_race != 0;
    // (both loops are wave-uniform and run every lane with `live` = busy - see Lane::iterate on why a finished or empty lane may
    // keep computing: a per-lane branch around the 2 600-instruction body costs exec-mask saves in SGPR pairs, which spill here)
    while (__builtin_popcountll(bm) > (fork_ok ? 32 : 0)) {
      const bool done = L.template iterate<LaneT::STEADY>(*QC_PARAMS_HERE(Pg), eqp, busy);
      busy = busy & !done;
      bm = __builtin_amdgcn_ballot_w64(busy);
    }
    int partner = lane;   // the lane racing on the same robot (itself: no race)
    // per-lane flags of the race, packed into one VGPR (as separate bools they live in SGPR pairs across the 2 600-instruction
    // body, and SGPR pairs that spill leave frame slots): bit 0 this lane still holds a result (its own robot's) that has to
    // reach the output, bit 1 it is a twin, bit 2 it brought its robot to the KKT point
    int role = mine ? 1 : 0;
    if (bm != 0) {
      // lanes whose own robot is finished store it straight from their registers (the output stock aliases Hessian planes that
      // are still being read; Rwb comes from memory) - their registers are about to carry somebody else's robot
      if (mine && !busy) {
        CParams& P = *QC_PARAMS_HERE(Pg);
        store_result<KIN, 4, false>(P, IN(), OUT(), L.idx, L.stance, L.status, L.iters, L.word_bits() | 0x80000000u, L.f, 0);
        role = 0;
      }
      const int nb = __builtin_popcountll(bm);
      const unsigned long long idle = ~bm;
      const int my_rank = (int)__builtin_amdgcn_mbcnt_hi((unsigned)((busy ? bm : idle) >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)(busy ? bm : idle), 0));
      // lane id of the rank-th set bit of m (ranks from 0; m has more than `rank` bits set): binary search on popcounts
      auto nth = [](unsigned long long m, int rank) {
        int pos = 0;
#pragma unroll
        for (int w = 32; w >= 1; w >>= 1) {
          const int c = __builtin_popcountll(m & ((1ull << w) - 1ull));
          const bool up = rank >= c;
          m = up ? (m >> w) : m;
          rank -= up ? c : 0;
          pos += up ? w : 0;
        }
        return pos;
      };
      const bool twin = !busy && my_rank < nb;  // the my_rank-th idle lane takes the my_rank-th running robot
      if (busy) partner = nth(idle, my_rank);
      if (twin) partner = nth(bm, my_rank);
      // the owner's state, read by its twin (every lane executes the shuffles; only twins keep what they read)
      const int src = twin ? partner : lane;
      auto take_i = [&](int v) { return __builtin_amdgcn_ds_bpermute(src << 2, v); };
      auto take_d = [&](double v) {
        const unsigned long long u = (unsigned long long)__double_as_longlong(v);
        const unsigned lo = (unsigned)take_i((int)(unsigned)u), hi = (unsigned)take_i((int)(unsigned)(u >> 32));
        return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
      };
      const uint32_t wbits = (uint32_t)take_i((int)L.word_bits());
      const uint32_t stance_o = (uint32_t)take_i((int)L.stance);
      const int iters_o = take_i(L.iters);
      const double tol_o = take_d(L.tol_s);
      const int idx_lo = take_i((int)(unsigned)(unsigned long long)L.idx), idx_hi = take_i((int)(unsigned)((unsigned long long)L.idx >> 32));
      // (one value at a time, selected in place: two dozen temporaries next to the 78-entry factor's registers would spill)
#pragma unroll
      for (int k = 0; k < 12; k++) {
        const double tf = take_d(L.f[k]);
        L.f[k] = twin ? tf : L.f[k];
        const double tc = take_d(eqp.c[k]);
        eqp.c[k] = twin ? tc : eqp.c[k];
      }
      if (twin) {
        L.stance = stance_o;
        L.iters = iters_o;
        L.idx = (long)(((unsigned long long)(unsigned)idx_hi << 32) | (unsigned)idx_lo);
        L.status = QC_MAX_ITER;
        L.tol_s = tol_o;
        L.have_f = true;
        L.drop_all = true;
        L.foot0 = 0;
#pragma unroll
        for (int i = 0; i < 4; i++) {
          const uint32_t fb = wbits >> (6 * i);
          L.C.sx[i] = dec2(fb); L.C.sy[i] = dec2(fb >> 2); L.C.sz[i] = dec2(fb >> 4);
        }
        // the robot's Hessian: the twin reads the owner's LDS column (read-only after setup; same address in both lanes = a broadcast)
        eqp.Qs = eqp.Qs - lane + partner;
        role = 2;
        busy = true;
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    asm volatile("" : "+v"(role), "+v"(partner));
    while (__builtin_amdgcn_ballot_w64(busy) != 0) {
      const bool done = L.template iterate<LaneT::STEADY>(*QC_PARAMS_HERE(Pg), eqp, busy);
      asm volatile("" : "+v"(role), "+v"(partner));
      const int solved = (busy && done && L.status == QC_SOLVED) ? 1 : 0;
      const int fin = (busy && done) ? 1 : 0;
      const int theirs = __builtin_amdgcn_ds_bpermute(partner << 2, solved);
      // a tie goes to the owner (the classic rule); a twin stops as soon as its owner is finished in any way
      const int owner_done = __builtin_amdgcn_ds_bpermute(partner << 2, fin);
      const bool is_twin = (role & 2) != 0;
      role |= (solved && !(is_twin && theirs)) ? 4 : 0;
      busy = busy && !done && !(partner != lane && theirs) && !(is_twin && owner_done);
    }
    // who stores: the owner, unless its twin got to the KKT point first (then the twin)
    const int twin_won = __builtin_amdgcn_ds_bpermute(partner << 2, ((role & 6) == 6) ? 1 : 0);
    const bool store_own = (role & 1) && !(partner != lane && twin_won);
    if (store_own || (role & 6) == 6) {  // straight from the registers, like the lanes that finished before the fork: no output stock on this path
      CParams& P = *QC_PARAMS_HERE(Pg);
      store_result<KIN, 4, false>(P, IN(), OUT(), L.idx, L.stance, L.status, L.iters, L.word_bits() | 0x80000000u, L.f, 0);
    }
    QC_CLK_END(8);
    return;
  } else {
    while (busy) {
      if constexpr (RESIDENT) {
        pin_uconst(uc);
        busy = !L.template iterate<LaneT::STEADY>(uc, eqp);
      } else {
        busy = !L.template iterate<LaneT::STEADY>(*QC_PARAMS_HERE(Pg), eqp);
      }
    }
    if constexpr (HESS_ONLY) __syncthreads();  // (the dense joint_q kernel) every lane is past its last read of the Hessian planes the output stock aliases
    if (mine) L.template push_result<SP>(sout, grp);
  }
  QC_CLK(7, 8);
  __syncthreads();
  flush_out<Eqp::G, KIN, STR, SP, RPARK>(Pg, IN(), OUT(), sout, stock_n, lane, RPARK ? sin : nullptr, QPARK ? sin + QPARK_Q * SP : nullptr);
  QC_CLK_END(8);
}



// ----------------------------------------------------------------------------------------------------------------
// MODE 3, paired waves (round 3): the one-lane kernel of batches that need more than one round of workgroups.
//
// A workgroup is TWO waves = 128 consecutive robots.  Each wave fills and takes its clamp steps exactly as the one-fill
// kernel does (one lane per robot, every load in one batch, Rwb parked in LDS), stores the robots that are finished straight
// from its registers, and writes the state of those still running - 33 doubles each - to a RECORD list in the
// workgroup's LDS.  Then it bumps an LDS counter: the wave that arrives FIRST simply ends (its wave slot is free for
// the next workgroup; nothing ever waits at a barrier after the first microsecond), the one that arrives LAST finishes
// both waves' stragglers four lanes per robot on the strided MFMA body, sixteen at a time, REFILLING lane groups from
// the list as robots finish, and races the two drop rules on the last <= 8 (cold batches).
// Why: in the one-fill kernel every wave finishes its own <= 16 stragglers and stays until the slowest is done - 5.65 tail
// recalculations per wave on config 5, mostly with a few of the 16 lane groups live.  Two waves' stragglers (~38 after
// five clamp steps) keep the 16 groups full for most of the walk: 4.8 tail recalculations per wave in the prototype
// (oracle/prototypes/proto_straggler_queue.py, K = 2) and no one-lane recalculation at 30 % occupancy in between.
// The same idea through a list in GLOBAL memory shared by K workgroups lost (tools/experiments/straggler_queue.patch: a
// memory round trip per refill, and a K-waves-long serial chain at the end of the launch); here a refill is a handful
// of ds_reads and the chain is two waves' worth.  And as ONE persistent wave that alternates fills and list consumption
// (tools/experiments/straggler_list_persistent.patch) it lost to code generation: a loop around the two heavy phases makes
// the compiler hoist invariants above bodies that need all 256 registers - scratch, whose first touch costs a wave ~10 us.
// Measured (profiles/r03_paired_waves.log): -5 % from four rounds of workgroups on (524 288 robots: 164 -> 156 us, 1 M: 300 ->
// 285, 2 M: 545 -> 515), nothing at two rounds - the early wave's slot idles until a second one is free for the next
// two-wave workgroup - which is where the planner draws the line.
constexpr int PAIR_REC = 33;    // doubles per record (odd: the records of the 16 lane groups fall into different banks):
                                // 0-5 -b, 6 {slot | stance << 8 | face codes << 24 | iters << 48}, 7-18 r, 19-30 f
                                // (PAIR_CAP, the records a wave may leave: qc_device.hpp, the planner clamps the threshold to it)
struct PairLds {
  double Rrows[128 * 9];                 // Rwb of the workgroup's robots, for the output transform
  double rec[2 * PAIR_CAP * PAIR_REC];   // the record list; once it is drained, the race stage's re-pack area
  int count[2], arrived;  // records in the list (paired: count[0]; solo: one list per wave)
};

template <class Eqp, bool KIN>
__global__ __launch_bounds__(128, 2) void balance_pair_kernel(const DevParams* __restrict__ Pg, const long n, const BatchIn in,
                                                              const uint32_t* __restrict__ warm, const BatchOut out, const int th,
                                                              const int refill, const int race, const unsigned solo_from) {
  static_assert(Eqp::G == 1 && Eqp::kNegB, "one lane per robot, 6x6 forms");
  static_assert(8 * REPACK_RS <= PAIR_CAP * PAIR_REC, "the race stage re-packs into the drained list (a solo wave's half of it)");
  constexpr bool UNIFORM = Eqp::kUniform;
  using Lane1 = Lane<Eqp, KIN>;
  using Eqp4 = EqpDiagW<UNIFORM, 4>;
  using Lane4 = Lane<Eqp4, KIN>;
  using LaneR = Lane<Eqp4, KIN, true>;  // with a per-lane drop rule
  __shared__ PairLds lds;
  const int lane = threadIdx.x & 63;
  const int slot = threadIdx.x;  // 0 ... 127: this robot's place in the workgroup (= its Rwb row)
  const long base = (long)blockIdx.x * 128;
  const long robot = base + slot;
  const bool mine = robot < n;
  QC_CLK_BEGIN();
  // SOLO: the workgroups of the launch's LAST round keep their stragglers to themselves - each wave is the consumer of its own
  // list.  Behind them no workgroup is waiting for a wave slot, so nothing is gained by ending early, and a wave's own list
  // is the shorter chain at the end of the launch.
  const bool solo = blockIdx.x >= solo_from;
  const int wv_id = threadIdx.x >> 6;
  if (threadIdx.x == 0) { lds.count[0] = 0; lds.count[1] = 0; lds.arrived = 0; }
  __syncthreads();  // the only barrier: both waves have just started
  double* const list = lds.rec + (solo ? wv_id * PAIR_CAP * PAIR_REC : 0);
  int* const list_n = &lds.count[solo ? wv_id : 0];
  // ---------------------------------------------------------------- producer: one lane per robot
  {
    Lane1 L;
    Eqp eqp(nullptr);
    L.idx = -1;
    L.foot0 = 0;
    L.stance = 0;
    L.tol_s = 0.0;
    bool busy = false;
    if (mine) {
      const uint32_t sw = in.stance ? *reinterpret_cast<const uint32_t*>(in.stance + 4 * robot) : 0u;
      const uint32_t wv = warm ? warm[robot] : 0u;
      RawState S;
      TickExtra X;
      double fp[12];
      fetch_extra<KIN>(in, robot, X);
      fetch_state<4, KIN>(in, robot, 0, S, fp);
      asm volatile("" ::: "memory");  // (every load of the fill is issued above this line)
      CParams& P = *QC_PARAMS_HERE(Pg);
      Wrench<4> W;
      const uint32_t st = assemble_from_state<KIN, 4, false>(P, in, robot, 0, S, fp, sw, X, W);
#pragma unroll
      for (int k = 0; k < 9; k++) lds.Rrows[9 * slot + k] = S.R[k];
      L.load_direct(W, st, wv, robot, 0, P.tol_start);
      eqp.setup(P, L.Wr, 0);
      busy = P.max_iter != 0;  // (0: the batch-load probe - load -> assemble -> store only)
    }
    QC_CLK(0, 2);
    const int first_steps = clamp_steps_for<1>(*QC_PARAMS_HERE(Pg), warm);
#pragma unroll 1
    for (int k = 0; k < first_steps; k++)
      if (busy) busy = !L.template iterate<Lane1::FIRST>(*QC_PARAMS_HERE(Pg), eqp, true, k == 0 && warm == nullptr);
    unsigned long long bm = __builtin_amdgcn_ballot_w64(busy);
    while (__builtin_popcountll(bm) > th) {
      if (busy) busy = !L.template iterate<Lane1::STEADY>(*QC_PARAMS_HERE(Pg), eqp);
      bm = __builtin_amdgcn_ballot_w64(busy);
    }
    if (mine && !busy) {
      CParams& P = *QC_PARAMS_HERE(Pg);
      store_result<KIN, 4, true>(P, in, out, robot, L.stance, L.status, L.iters, L.word_bits() | 0x80000000u, L.f, 0, lds.Rrows + 9 * slot, 1);
    }
    const int nb = __builtin_popcountll(bm);
    int first = 0;
    if (nb > 0 && lane == 0) first = __hip_atomic_fetch_add(list_n, nb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    first = __builtin_amdgcn_readfirstlane(first);
    if (busy) {
      const int rank = __builtin_amdgcn_mbcnt_hi((unsigned)(bm >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bm, 0));
      double* rec = list + (first + rank) * PAIR_REC;
#pragma unroll
      for (int k = 0; k < 6; k++) rec[k] = L.Wr.b[k];
      const unsigned long long fl = (unsigned long long)slot | ((unsigned long long)((L.stance | L.polish_bit()) & 0x3FFu) << 8) |
                                    ((unsigned long long)(L.word_bits() & 0xFFFFFFu) << 24) | ((unsigned long long)(uint32_t)L.iters << 48);
      rec[6] = __longlong_as_double((long long)fl);
#pragma unroll
      for (int i = 0; i < 4; i++)
#pragma unroll
        for (int k = 0; k < 3; k++) {
          rec[7 + 3 * i + k] = L.Wr.r[i][k];
          rec[19 + 3 * i + k] = L.f[3 * i + k];
        }
    }
  }
  // ---------------------------------------------------------------- hand-over inside the workgroup: the last wave to arrive consumes
  int arrived = 1;
  if (!solo) {
    if (lane == 0) arrived = __hip_atomic_fetch_add(&lds.arrived, 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_WORKGROUP);
    arrived = __builtin_amdgcn_readfirstlane(arrived);
  }
  if (arrived == 0) return;  // (no clock hook here: the development harnesses' end-of-kernel hooks may hold a barrier)
  const int T = __hip_atomic_load(list_n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  if (T == 0) {
    QC_CLK_END(8);
    return;
  }
  QC_CLK(7, 8);
  // ---------------------------------------------------------------- consumer: four lanes per robot, refilled from the list
  const int g4 = lane & 15, j4 = lane >> 4;
  Lane4 L4;
  Eqp4 eqp4(nullptr);
  int rslot = 0;  // the robot's place in the workgroup (its Rwb row)
  auto take = [&](int t) {
    const double* rec = list + t * PAIR_REC;
#pragma unroll
    for (int k = 0; k < 6; k++) {
      L4.Wr.b[k] = rec[k];  // (already -b)
      asm volatile("" : "+v"(L4.Wr.b[k]));
    }
    const unsigned long long fl = (unsigned long long)__double_as_longlong(rec[6]);
#pragma unroll
    for (int k = 0; k < 3; k++) {
      L4.Wr.r[0][k] = rec[7 + 3 * j4 + k];
      L4.f[k] = rec[19 + 3 * j4 + k];
    }
    rslot = (int)(fl & 0xFFu);
    L4.idx = base + rslot;
    L4.stance = (uint32_t)((fl >> 8) & 0x1FFu);
    const uint32_t fw = (uint32_t)(fl >> (24 + 6 * j4));
    L4.iters = (int)(fl >> 48);
    L4.foot0 = j4;
    L4.set_foot_code(0, fw);
    if constexpr (Lane4::kArith) L4.set_face_const(*QC_PARAMS_HERE(Pg));
    L4.status = QC_MAX_ITER;
    {
      const double tol = Lane4::kTol * QC_PARAMS_HERE(Pg)->tol_d;
      L4.tol_s = ((fl >> 8) & QC_POLISH_ONE) ? tol : -tol;
    }
    L4.have_f = true;
    eqp4.setup(*QC_PARAMS_HERE(Pg), L4.Wr, j4);
  };
  auto push4 = [&](const Lane4& X, int rs) {  // this lane's foot of a finished robot, straight to the outputs
    const uint32_t word = (uint32_t)group_or<4, true>((int)X.word_bits()) | 0x80000000u;
    CParams& P = *QC_PARAMS_HERE(Pg);
    store_result<KIN, 1, true>(P, in, out, X.idx, X.stance, X.status, X.iters, word, X.f, j4, lds.Rrows + 9 * rs, 1);
  };
  // groups without a robot shadow ticket 0 (the strided layout keeps every lane in the loop: MFMA sums read all 64)
  bool busy4 = g4 < T;
  bool holds = busy4;  // the group holds a robot whose result has not been stored yet
  take(busy4 ? g4 : 0);
  int next = T < 16 ? T : 16;
  const int stop = race ? 8 : 0;
  UConst uc;
  if constexpr (UNIFORM) uc = load_uconst(*QC_PARAMS_HERE(Pg));
  for (;;) {
    bool done;
    if constexpr (UNIFORM) {
      pin_uconst(uc);
      done = L4.template iterate<Lane4::STEADY>(uc, eqp4, busy4);
    } else {
      done = L4.template iterate<Lane4::STEADY>(*QC_PARAMS_HERE(Pg), eqp4, busy4);
    }
    busy4 = busy4 & !done;
    const unsigned run16 = (unsigned)(__builtin_amdgcn_ballot_w64(busy4) & 0xFFFFull);  // member 0 of the groups = lanes 0-15
    const int nrun = __builtin_popcount(run16);
    if (next < T) {
      if (16 - nrun >= refill) {
        if (holds && !busy4) push4(L4, rslot);
        const unsigned free16 = ~run16 & 0xFFFFu;
        const int t = next + __builtin_popcount(free16 & ((1u << g4) - 1u));
        if (!busy4) {
          holds = t < T;
          if (holds) {
            take(t);
            busy4 = true;
          }
        }
        next += __builtin_popcount(free16);
        next = next < T ? next : T;
      }
      continue;
    }
    if (nrun <= stop) break;
  }
  if (holds && !busy4) push4(L4, rslot);
  const unsigned run16 = (unsigned)(__builtin_amdgcn_ballot_w64(busy4) & 0xFFFFull);
  const int nrun = __builtin_popcount(run16);
  if (nrun == 0) {
    QC_CLK_END(8);
    return;
  }
  // race stage (as the one-fill kernels' tail): the <= 8 survivors are re-packed - through the drained list - each into TWO
  // groups 8 lanes apart that continue with different drop rules (most negative multiplier / all negative multipliers);
  // the first at the KKT point wins
  {
    double* rpk = list;
    const int rank = __builtin_popcount(run16 & ((1u << g4) - 1u));
    __builtin_amdgcn_wave_barrier();  // (this wave is alone by now; LDS operations of one wave stay in order)
    if (busy4) repack_write(L4, rpk + rank * REPACK_RS, rslot, j4);
    __builtin_amdgcn_wave_barrier();
    LaneR LR;
    Eqp4 eqpR(nullptr);
    const int r = g4 & 7, sid = g4 >> 3;  // robot, strategy of this group
    bool busyR = r < nrun;
    const int rs = repack_read(Pg, LR, eqpR, rpk + (busyR ? r : 0) * REPACK_RS, j4);
    LR.drop_all = sid == 1;
    unsigned solved_mask = 0;
    auto after = [&](bool fin) {
      const int me = (busyR & LR.kkt) ? (1 << sid) : 0;
      const int m = race_or<8, 2>(me);
      solved_mask |= (unsigned)m;
      busyR = busyR & !fin & (solved_mask == 0);
    };
    while (__builtin_amdgcn_ballot_w64(busyR) != 0) {
      if constexpr (UNIFORM) {
        pin_uconst(uc);
        after(LR.template iterate<LaneR::STEADY>(uc, eqpR, busyR));
      } else {
        after(LR.template iterate<LaneR::STEADY>(*QC_PARAMS_HERE(Pg), eqpR, busyR));
      }
    }
    const int win = solved_mask ? __builtin_ctz(solved_mask) : 0;
    if (r < nrun && sid == win) {
      const uint32_t word = (uint32_t)group_or<4, true>((int)LR.word_bits()) | 0x80000000u;
      CParams& P = *QC_PARAMS_HERE(Pg);
      store_result<KIN, 1, true>(P, in, out, LR.idx, LR.stance, LR.status, LR.iters, word, LR.f, j4, lds.Rrows + 9 * rs, 1);
    }
  }
  QC_CLK_END(8);
}

}  // namespace qc

// =============================================================== host / C ABI
typedef void (*qc_kernel_fn)(const qc::DevParams*, long, qc::BatchIn, const uint32_t*, qc::BatchOut, long);

// qc::BalanceKernelArgs is a hand-written mirror of balance_kernel's parameter list (the kernarg segment lays every argument at the
// next multiple of its alignment); every instantiation is stored as a qc_kernel_fn, so that type IS the list.  Growing BatchIn or
// BatchOut moves the members behind it: these asserts fail the build instead of letting kernarg_here read the wrong bytes.
template <class... A>
constexpr size_t kernarg_offset(int i) {
  constexpr size_t sz[] = {sizeof(A)...}, al[] = {alignof(A)...};
  size_t off = 0;
  for (int k = 0; k < (int)sizeof...(A); k++) {
    off = (off + al[k] - 1) / al[k] * al[k];
    if (k == i) return off;
    off += sz[k];
  }
  return off;
}
template <class F>
struct KernargOf;
template <class... A>
struct KernargOf<void (*)(A...)> {
  static constexpr int count = (int)sizeof...(A);
  static constexpr size_t at(int i) { return kernarg_offset<A...>(i); }
};
using KernelArgList = KernargOf<qc_kernel_fn>;
static_assert(KernelArgList::count == 6, "balance_kernel's parameter list changed: update qc::BalanceKernelArgs");
static_assert(offsetof(qc::BalanceKernelArgs, Pg) == KernelArgList::at(0) && offsetof(qc::BalanceKernelArgs, n) == KernelArgList::at(1) &&
                  offsetof(qc::BalanceKernelArgs, in) == KernelArgList::at(2) && offsetof(qc::BalanceKernelArgs, warm) == KernelArgList::at(3) &&
                  offsetof(qc::BalanceKernelArgs, out) == KernelArgList::at(4) && offsetof(qc::BalanceKernelArgs, chunk) == KernelArgList::at(5),
              "qc::BalanceKernelArgs no longer mirrors balance_kernel's kernarg layout");
static_assert(sizeof(qc::CertifySummary) == sizeof(qc_certify_summary) && offsetof(qc::CertifySummary, worst_primal) == offsetof(qc_certify_summary, worst_primal) &&
                  offsetof(qc::CertifySummary, arg_stationarity) == offsetof(qc_certify_summary, arg_stationarity),
              "qc::CertifySummary mirrors qc_certify_summary");
static_assert(qc::PARAM_COUNT == QC_PARAM_COUNT && offsetof(qc_params, max_iter) == sizeof(double) * QC_PARAM_COUNT,
              "QC_PARAM_COUNT is the number of doubles of qc_params, in its order");
static_assert(sizeof(qc::CmdState) == sizeof(qc_commander_state) && offsetof(qc::CmdState, Vb) == offsetof(qc_commander_state, Vb) &&
                  offsetof(qc::CmdState, Rwb_d) == offsetof(qc_commander_state, Rwb_d) && offsetof(qc::CmdState, w_d) == offsetof(qc_commander_state, w_d),
              "qc::CmdState mirrors qc_commander_state");

struct qc_handle {
  int device = 0;
  int cus = 0;  // compute units of the device
  qc::DevParams dp;
  qc::DevParams* d_params = nullptr;  // device copy of dp (rewritten only by the qc_set_* calls, after a device synchronise)
  qc::Tuning tune;
  long resident[qc::N_KERNELS][2] = {};  // resident_workgroups' answers per kernel and joint_q variant, 0 = not asked yet
  // staging buffers for the host-pointer entry points
  void* stage = nullptr;
  size_t stage_bytes = 0;
  void* pin = nullptr;  // pinned host buffer the kernel reads/writes in place for small batches
  size_t pin_bytes = 0;
  uint32_t last_word = 0;  // qc_control(): working set of the previous call (hot start)
  bool has_last = false;
  hipStream_t stream = nullptr;
  qc::CertifySummary* certify_parts = nullptr;  // qc_certify_batch: one partial per workgroup of certify_kernel (CERTIFY_MAX_PARTIALS)
  double* com_parts = nullptr;    // qc_com_reference_adjoint_batch: one partial of 16 doubles per workgroup (COM_SUM_MAX_BLOCKS)
  double* param_parts = nullptr;  // qc_sensitivity_param_batch: one partial of PARAM_COUNT doubles per workgroup (SENSITIVITY_PARAM_MAX_BLOCKS)
};

using qc::fail;
#define QC_HIP(expr)                                                                      \
  do {                                                                                    \
    hipError_t e_ = (expr);                                                               \
    if (e_ != hipSuccess) return fail(QC_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
  } while (0)

// Rewrites the device copy of the constants.  Launches in flight - on any stream, non-blocking ones included -
// may still be reading the old copy through scalar loads, so the device is drained first; the copy itself is
// synchronous.  Setters are configuration calls, not per-tick calls.
static int upload_params(qc_handle* h) {
  QC_HIP(hipSetDevice(h->device));
  QC_HIP(hipDeviceSynchronize());
  QC_HIP(hipMemcpy(h->d_params, &h->dp, sizeof(qc::DevParams), hipMemcpyHostToDevice));
  return QC_OK;
}

// ---------------------------------------------------------------- the kernel table
typedef void (*qc_pair_kernel_fn)(const qc::DevParams*, long, qc::BatchIn, const uint32_t*, qc::BatchOut, int, int, int, unsigned);
// the EQP struct that solves a form on G lanes per robot
template <int FORM, int G>
struct EqpOf { using type = qc::EqpDiagW<FORM == qc::QC_FORM_UNIFORM, G>; };
template <>
struct EqpOf<qc::QC_FORM_DENSE, 4> { using type = qc::EqpDense4; };
template <>
struct EqpOf<qc::QC_FORM_DENSE, 1> { using type = qc::EqpDense; };

// One row per key of qc::KERNEL_KEYS (same index): the instantiation's entry points without and with joint_q and the dynamic LDS each
// is launched with (qc::LdsLayout, which the kernel addresses by), or the paired-waves one (mode 3; static LDS, QP only).
struct qc_kernel_row {
  qc_kernel_fn fn[2];  // [joint_q]
  size_t lds[2];
  qc_pair_kernel_fn pfn;  // mode 3
};
template <int I>
static qc_kernel_row kernel_row() {
  constexpr qc::KernelKey k = qc::KERNEL_KEYS[I];
  using EQP = typename EqpOf<k.form, k.G>::type;
  constexpr int MINW = k.form == qc::QC_FORM_DENSE ? 1 : 2;
  if constexpr (k.mode == 3) {
    return qc_kernel_row{{nullptr, nullptr}, {0, 0}, (qc_pair_kernel_fn)qc::balance_pair_kernel<EQP, false>};
  } else {
    qc_kernel_row r{{nullptr, nullptr}, {qc::LdsLayout<EQP, false, k.mode>::BYTES, qc::LdsLayout<EQP, true, k.mode>::BYTES}, nullptr};
    r.fn[1] = (qc_kernel_fn)qc::balance_kernel<EQP, true, MINW, k.mode, k.race>;
    r.fn[0] = (qc_kernel_fn)qc::balance_kernel<EQP, false, MINW, k.mode, k.race>;
    return r;
  }
}
template <int... I>
static const qc_kernel_row& kernel_row_at(int kernel, std::integer_sequence<int, I...>) {
  static const qc_kernel_row rows[] = {kernel_row<I>()...};
  return rows[kernel];
}
static const qc_kernel_row& kernel_row_at(int kernel) { return kernel_row_at(kernel, std::make_integer_sequence<int, qc::N_KERNELS>()); }

// workgroups of a kernel (its joint_q variant with `kin`) the device holds at once: registers, LDS and the 32-waves-per-CU cap, as
// the runtime sees them
static long resident_workgroups(qc_handle* h, int kernel, bool kin) {
  if (h->tune.wave_slots_override > 0) return h->tune.wave_slots_override;
  long& r = h->resident[kernel][kin];
  if (r == 0) {
    const qc_kernel_row& k = kernel_row_at(kernel);
    int per_cu = 0;
    const hipError_t e = k.pfn ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void*)k.pfn, 128, 0)
                               : hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void*)k.fn[kin], 64, k.lds[kin]);
    if (e != hipSuccess || per_cu <= 0) per_cu = 4;
    r = (long)per_cu * h->cus;
  }
  return r;
}

// the planner (qc_host.hpp) on a handle's form, tuning and device
static int plan_launch(qc_handle* h, long n, bool kin, bool warm, qc::LaunchPlan* lp) {
  return qc::plan_launch(qc::form_of(h->tune), n, kin, warm, h->tune, h->cus, [h](int kernel, bool k) { return resident_workgroups(h, kernel, k); }, lp);
}

// how every qc_default_* opens: the record zeroed and its struct_size set; false for a null record
template <class Io>
static bool zeroed(Io* io) {
  if (!io) return false;
  std::memset(io, 0, sizeof(Io));
  io->struct_size = sizeof(Io);
  return true;
}

// What the certificate and the adjoint kernels read of a qc_batch_in: what the solve reads minus everything that advances or plans
// (gait_dt, swing_*) - nothing of `in` is written.  mask = false drops the contact-mask arrays too (stance, gait_phase, gait_duty).
static qc::BatchIn readonly_view(const qc_batch_in* in, bool mask) {
  return qc::BatchIn{in->Rwb, in->Rwb_d, in->x, in->xdot, in->w, in->x_d, in->xdot_d, in->w_d, in->feet, mask ? in->stance : nullptr, in->joint_q,
                     mask ? in->gait_phase : nullptr, mask ? in->gait_duty : nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
}

// one launch of a kernel without dynamic LDS on a flat grid, checked
template <class... P, class... A>
static int launch_flat(void (*kernel)(P...), unsigned blocks, int block, void* stream, const A&... args) {
  kernel<<<dim3(blocks), dim3(block), 0, (hipStream_t)stream>>>(args...);
  QC_HIP(hipGetLastError());
  return QC_OK;
}

// one launch of a `template <bool KIN>` per-robot kernel - `kin` where `bi` carries joint_q, `feet` where it does not -, checked
template <class Args>
static int launch_per_robot(void (*kin)(const qc::DevParams*, long, qc::BatchIn, Args), void (*feet)(const qc::DevParams*, long, qc::BatchIn, Args),
                            unsigned blocks, int block, const qc_handle* h, size_t n, const qc::BatchIn& bi, const Args& a, void* stream) {
  return launch_flat(bi.joint_q ? kin : feet, blocks, block, stream, h->d_params, (long)n, bi, a);
}

// the instantiation of a `template <bool, bool>` kernel that two flags of the call pick
template <class Fn>
static Fn pick2(bool first, bool second, Fn tt, Fn tf, Fn ft, Fn ff) {
  return first ? (second ? tt : tf) : (second ? ft : ff);
}

extern "C" {

const char* qc_last_error(void) { return qc::g_err.c_str(); }
int qc_abi_version(void) { return QC_ABI_VERSION; }
int qc_check_abi(int abi_version, size_t sizeof_params, size_t sizeof_batch_in, size_t sizeof_batch_out) {
  // A caller compiled against another revision of include/qc_balance.h would hand over structs of another size
  // (qc_batch_in has grown with every ABI revision and carries no size field): refuse it before any of them is read.
  if (abi_version != QC_ABI_VERSION || sizeof_params != sizeof(qc_params) || sizeof_batch_in != sizeof(qc_batch_in) ||
      sizeof_batch_out != sizeof(qc_batch_out)) {
    char msg[256];
    std::snprintf(msg, sizeof(msg), "qc_check_abi: caller built against ABI v%d (qc_params %zu B, qc_batch_in %zu B, qc_batch_out %zu B), library is "
                  "ABI v%d (%zu / %zu / %zu B)", abi_version, sizeof_params, sizeof_batch_in, sizeof_batch_out, QC_ABI_VERSION,
                  sizeof(qc_params), sizeof(qc_batch_in), sizeof(qc_batch_out));
    return fail(QC_ERR_ABI, msg);
  }
  return QC_OK;
}
const char* qc_kernel_name(const qc_handle* h) {
  if (!h) return "";
  static const char* const names[] = {"diagW-6x6-uniform", "diagW-6x6", "dense-12x12"};  // QC_FORM_*
  return names[qc::form_of(h->tune)];
}

void qc_default_kinematics(qc_kinematics* k) { qc::default_kinematics(k); }

void qc_swing_state_init(qc_swing_state* s, size_t n) {
  if (!s) return;
  std::memset(s, 0, n * sizeof(qc_swing_state));
  for (size_t i = 0; i < n; i++)
    for (int l = 0; l < 4; l++) s[i].leg_state[l] = -1;
}

void qc_default_command(qc_command_in* c) {
  if (!zeroed(c)) return;
  c->stand_height = 0.26;  // x_stand(2), commander_node.cpp:355
  c->stand_tol = 0.005;    // commander_node.cpp:387
  c->cmd_dt = 0.001;       // "User cmd integration step", commander_node.cpp:344
}

void qc_commander_state_init(qc_commander_state* s, size_t n, const double x_stand[3]) {
  if (!s) return;
  const double xs[3] = {x_stand ? x_stand[0] : 0.0, x_stand ? x_stand[1] : 0.0, x_stand ? x_stand[2] : 0.26};  // :354
  std::memset(s, 0, n * sizeof(qc_commander_state));
  for (size_t i = 0; i < n; i++) {
    s[i].Rwb_d[0] = s[i].Rwb_d[4] = s[i].Rwb_d[8] = 1.0;  // Rwb_d = eye(3, 3), :347
    for (int k = 0; k < 3; k++) s[i].x_d[k] = xs[k];      // x_d = x_stand, :364
  }
}

int qc_set_kinematics(qc_handle* h, const qc_kinematics* kin) {
  if (!h) return fail(QC_ERR_INVALID, "qc_set_kinematics: null handle");
  qc_kinematics k;
  if (kin) k = *kin; else qc::default_kinematics(&k);
  if (!(k.tau_min <= k.tau_max)) return fail(QC_ERR_INVALID, "qc_set_kinematics: need tau_min <= tau_max");
  qc::copy_kinematics(h->dp, k);
  return upload_params(h);
}

int qc_set_gait(qc_handle* h, double t_swing, double t_stance) {
  if (!h) return fail(QC_ERR_INVALID, "qc_set_gait: null handle");
  if (!(t_swing >= 0.0) || !(t_stance >= 0.0) || !(t_swing + t_stance > 0.0)) return fail(QC_ERR_INVALID, "qc_set_gait: need t_swing, t_stance >= 0, not both 0");
  h->dp.stance_phase = t_stance / (t_swing + t_stance);  // gait.cpp:45
  h->dp.t_swing = t_swing;
  h->dp.t_stance = t_stance;
  return upload_params(h);
}

int qc_create_abi(const qc_params* p, int device, qc_handle** out, int abi_version, size_t sizeof_params, size_t sizeof_batch_in,
                  size_t sizeof_batch_out) {
  if (!p || !out) return fail(QC_ERR_INVALID, "qc_create: null argument");
  *out = nullptr;
  // ABI v6: no handle for a caller that fills other structs than this library reads (include/qc_balance.h, qc_create)
  if (const int rc = qc_check_abi(abi_version, sizeof_params, sizeof_batch_in, sizeof_batch_out); rc != QC_OK) return rc;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(QC_ERR_NO_DEVICE, "qc_create: no HIP device visible (this library has no CPU path)");
  if (device < 0 || device >= ndev) return fail(QC_ERR_INVALID, "qc_create: device ordinal out of range");
  if (const int rc = qc::check_params(p); rc != QC_OK) return rc;
  qc_handle* h = new (std::nothrow) qc_handle();
  if (!h) return fail(QC_ERR_INVALID, "qc_create: out of memory");
  h->device = device;
  // (from here on a failure goes through qc_destroy, which frees whatever is there - and, as a qc_create that succeeds does, leaves
  // `device` the calling thread's current device)
  if (const int rc = qc::derive_params(p, h->dp, h->tune); rc != QC_OK) { qc_destroy(h); return rc; }
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess) { qc_destroy(h); return fail(QC_ERR_HIP, "qc_create: hipGetDeviceProperties failed"); }
  h->cus = prop.multiProcessorCount;
  if (hipSetDevice(device) != hipSuccess || hipMalloc((void**)&h->d_params, sizeof(qc::DevParams)) != hipSuccess ||
      hipMemcpy(h->d_params, &h->dp, sizeof(qc::DevParams), hipMemcpyHostToDevice) != hipSuccess) {
    qc_destroy(h);
    return fail(QC_ERR_HIP, "qc_create: could not upload the controller constants");
  }
  // The handle-owned partial buffers of qc_certify_batch (224 KB), qc_sensitivity_param_batch (1.7 MB) and
  // qc_com_reference_adjoint_batch (128 KB), allocated here and not at the first call: that call may be inside a graph capture.
  const struct { void** member; size_t bytes; const char* message; } parts[] = {
      {(void**)&h->certify_parts, sizeof(qc::CertifySummary) * qc::CERTIFY_MAX_PARTIALS, "qc_create: could not allocate the certificate's partial buffer"},
      {(void**)&h->param_parts, sizeof(double) * qc::PARAM_COUNT * qc::SENSITIVITY_PARAM_MAX_BLOCKS, "qc_create: could not allocate the parameter cotangents' partial buffer"},
      {(void**)&h->com_parts, sizeof(double) * 16 * qc::COM_SUM_MAX_BLOCKS, "qc_create: could not allocate the schedule cotangent's partial buffer"}};
  for (const auto& part : parts)
    if (hipMalloc(part.member, part.bytes) != hipSuccess) {
      qc_destroy(h);
      return fail(QC_ERR_HIP, part.message);
    }
  *out = h;
  return QC_OK;
}

int qc_set_tuning(qc_handle* h, const char* key, double value) {
  if (!h || !key) return fail(QC_ERR_INVALID, "qc_set_tuning: null argument");
  bool upload = false;
  if (const int rc = qc::set_tuning(h->tune, h->dp, key, value, &upload); rc != QC_OK) return rc;
  return upload ? upload_params(h) : QC_OK;
}

int qc_query_launch(qc_handle* h, size_t n, int kin, int warm, qc_launch_info* out) {
  if (!h || !out) return fail(QC_ERR_INVALID, "qc_query_launch: null argument");
  QC_HIP(hipSetDevice(h->device));
  qc::LaunchPlan lp;
  const int rc = plan_launch(h, (long)(n ? n : 1), kin != 0, warm != 0, &lp);
  if (rc != QC_OK) return rc;
  const qc::KernelKey& k = qc::KERNEL_KEYS[lp.kernel];
  out->lanes_per_robot = k.G;
  out->mode = k.mode;
  out->form = k.form;
  out->strategies = k.race;
  out->chunk = lp.chunk;
  out->blocks = lp.blocks;
  out->resident_workgroups = resident_workgroups(h, lp.kernel, kin != 0);
  out->lds_bytes = (int64_t)kernel_row_at(lp.kernel).lds[kin != 0];
  return QC_OK;
}

void qc_destroy(qc_handle* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  if (h->d_params) (void)hipFree(h->d_params);
  if (h->certify_parts) (void)hipFree(h->certify_parts);
  if (h->param_parts) (void)hipFree(h->param_parts);
  if (h->com_parts) (void)hipFree(h->com_parts);
  if (h->stage) (void)hipFree(h->stage);
  if (h->pin) (void)hipHostFree(h->pin);
  if (h->stream) (void)hipStreamDestroy(h->stream);
  delete h;
}

// the one launch behind qc_control_batch and qc_tick_batch (arguments validated)
static int launch_batch(qc_handle* h, size_t n, bool kin, const qc::BatchIn& bi, const uint32_t* warm, const qc::BatchOut& bo, void* stream) {
  qc::LaunchPlan lp;
  const int rc = plan_launch(h, (long)n, kin, warm != nullptr, &lp);
  if (rc != QC_OK) return rc;
  const qc_kernel_row& r = kernel_row_at(lp.kernel);
  if (r.pfn) {  // mode 3
    // the last round of workgroups (those behind which nothing waits for a slot) runs solo
    const long solo_from = h->tune.pair_solo == 0 ? (long)lp.blocks : ((long)lp.blocks > lp.resident ? (long)lp.blocks - lp.resident : 0);
    r.pfn<<<dim3(lp.blocks), dim3(128), 0, (hipStream_t)stream>>>(h->d_params, (long)n, bi, warm, bo, lp.p_th, lp.p_refill,
                                                                  h->dp.tail_race && warm == nullptr ? 1 : 0, (unsigned)solo_from);
    QC_HIP(hipGetLastError());
    return QC_OK;
  }
  r.fn[kin]<<<dim3(lp.blocks), dim3(64), r.lds[kin], (hipStream_t)stream>>>(h->d_params, (long)n, bi, warm, bo, lp.chunk);
  QC_HIP(hipGetLastError());
  return QC_OK;
}

int qc_control_batch(qc_handle* h, size_t n, const qc_batch_in* in, const uint32_t* warm, const qc_batch_out* out, void* stream) {
  if (const int rc = qc::check_batch_args("qc_control_batch", h, n, in, out, true); rc != QC_OK || n == 0) return rc;
  QC_HIP(hipSetDevice(h->device));
  const bool kin = in->joint_q != nullptr;
  if (const int rc = qc::check_swing_gait_args(in, out); rc != QC_OK) return rc;
  qc::BatchIn bi{in->Rwb, in->Rwb_d, in->x, in->xdot, in->w, in->x_d, in->xdot_d, in->w_d, in->feet, in->stance, in->joint_q,
                 in->gait_phase, in->gait_duty, in->swing_pos, in->swing_vel, in->joint_qdot,
                 reinterpret_cast<qc::SwingState*>(in->swing_state), in->gait_dt};
  qc::BatchOut bo{out->grf_body, out->status, out->active_set, out->iterations, out->joint_tau};
  return launch_batch(h, n, kin, bi, warm, bo, stream);
}

int qc_tick_batch(qc_handle* h, size_t n, const qc_batch_in* in, const qc_command_in* cmd, const uint32_t* warm, const qc_batch_out* out,
                  void* stream) {
  if (const int rc = qc::check_tick_args(h, in, cmd, out); rc != QC_OK) return rc;
  if (n == 0) return QC_OK;
  QC_HIP(hipSetDevice(h->device));
  qc::BatchIn bi{in->Rwb, nullptr, in->x, in->xdot, in->w, nullptr, nullptr, nullptr, in->feet, nullptr, in->joint_q,
                 in->gait_phase, in->gait_duty, nullptr, nullptr, in->joint_qdot,
                 reinterpret_cast<qc::SwingState*>(in->swing_state), in->gait_dt,
                 reinterpret_cast<qc::CmdState*>(cmd->state), cmd->fresh ? cmd->twist : nullptr, cmd->fresh,
                 cmd->stand_height, cmd->stand_tol, cmd->cmd_dt};
  qc::BatchOut bo{out->grf_body, out->status, out->active_set, out->iterations, out->joint_tau};
  return launch_batch(h, n, true, bi, warm, bo, stream);
}

void qc_default_plant(qc_plant_io* io) {
  if (!zeroed(io)) return;
  io->dt = 1.0 / 300.0;  // mit_cheetah_config.yaml:3
}

int qc_plant_step_batch(qc_handle* h, size_t n, const qc_plant_io* io, void* stream) {
  if (const int rc = qc::check_plant_args(h, n, io); rc != QC_OK || n == 0) return rc;
  qc::PlantArgs a;
  if (const int rc = qc::plant_constants(h->dp.mass, h->dp.Ib, io, a); rc != QC_OK) return rc;
  QC_HIP(hipSetDevice(h->device));
  const unsigned blocks = (unsigned)((n + qc::PLANT_BLOCK - 1) / qc::PLANT_BLOCK);
  return launch_flat(qc::plant_step_kernel, blocks, qc::PLANT_BLOCK, stream, (long)n, a);
}

void qc_default_plant_adjoint(qc_plant_adjoint_io* io) {
  if (!zeroed(io)) return;
  io->dt = 1.0 / 300.0;  // qc_default_plant's
}

int qc_plant_step_adjoint_batch(qc_handle* h, size_t n, const qc_plant_adjoint_io* io, void* stream) {
  if (const int rc = qc::check_plant_adjoint_args(h, n, io); rc != QC_OK || n == 0) return rc;
  qc::PlantAdjointArgs a;
  if (const int rc = qc::plant_adjoint_constants(h->dp.mass, h->dp.Ib, io, a); rc != QC_OK) return rc;
  QC_HIP(hipSetDevice(h->device));
  const unsigned blocks = (unsigned)((n + qc::PLANT_BLOCK - 1) / qc::PLANT_BLOCK);
  return launch_flat(qc::plant_step_adjoint_kernel, blocks, qc::PLANT_BLOCK, stream, (long)n, a);
}

void qc_default_leg_plant(qc_leg_plant_io* io) {
  if (!zeroed(io)) return;  // (leg_inertia 0: the reference has no number for it, the caller gives one)
  io->dt = 1.0 / 300.0;  // mit_cheetah_config.yaml:3
}

int qc_leg_plant_step_batch(qc_handle* h, size_t n, const qc_leg_plant_io* io, void* stream) {
  if (const int rc = qc::check_leg_plant_args(h, n, io); rc != QC_OK || n == 0) return rc;
  qc::LegPlantArgs a;
  if (const int rc = qc::leg_plant_constants(h->dp.mass, h->dp.Ib, io, a); rc != QC_OK) return rc;
  QC_HIP(hipSetDevice(h->device));
  const unsigned blocks = (unsigned)((n + qc::LEG_PLANT_BLOCK - 1) / qc::LEG_PLANT_BLOCK);
  return launch_flat(qc::leg_plant_step_kernel, blocks, qc::LEG_PLANT_BLOCK, stream, h->d_params, (long)n, a);
}

void qc_default_leg_plant_adjoint(qc_leg_plant_adjoint_io* io) {
  if (!zeroed(io)) return;  // (leg_inertia 0, as qc_default_leg_plant leaves it)
  io->dt = 1.0 / 300.0;  // qc_default_leg_plant's
}

int qc_leg_plant_step_adjoint_batch(qc_handle* h, size_t n, const qc_leg_plant_adjoint_io* io, void* stream) {
  if (const int rc = qc::check_leg_plant_adjoint_args(h, n, io); rc != QC_OK || n == 0) return rc;
  qc::LegPlantAdjointArgs a;
  if (const int rc = qc::leg_plant_adjoint_constants(h->dp.mass, h->dp.Ib, io, a); rc != QC_OK) return rc;
  QC_HIP(hipSetDevice(h->device));
  const unsigned blocks = (unsigned)((n + qc::LEG_PLANT_BLOCK - 1) / qc::LEG_PLANT_BLOCK);
  return launch_flat(qc::leg_plant_step_adjoint_kernel, blocks, qc::LEG_PLANT_BLOCK, stream, h->d_params, (long)n, a);
}

void qc_default_plant_model(qc_plant_model* model) { (void)zeroed(model); }
void qc_default_plant_model_bar(qc_plant_model_bar* bar) { (void)zeroed(bar); }

// the instantiation <MASS, IB, WRENCH> of a model kernel for plant_model_variant()'s word (1 ... 7)
#define QC_MODEL_KERNELS(kernel)                                                                                                      \
  {nullptr, qc::kernel<true, false, false>, qc::kernel<false, true, false>, qc::kernel<true, true, false>, qc::kernel<false, false, true>, \
   qc::kernel<true, false, true>, qc::kernel<false, true, true>, qc::kernel<true, true, true>}

int qc_plant_step_model_batch(qc_handle* h, size_t n, const qc_plant_io* io, const qc_plant_model* model, void* stream) {
  if (const int rc = qc::check_plant_model_args(h, n, io, model); rc != QC_OK || n == 0) return rc;
  qc::PlantArgs a;
  if (const int rc = qc::plant_model_constants(h->dp.mass, h->dp.Ib, io, model, a); rc != QC_OK) return rc;
  QC_HIP(hipSetDevice(h->device));
  static void (*const kernels[8])(long, qc::PlantArgs, qc::PlantModelArgs) = QC_MODEL_KERNELS(plant_step_model_kernel);
  const unsigned blocks = (unsigned)((n + qc::PLANT_BLOCK - 1) / qc::PLANT_BLOCK);
  return launch_flat(kernels[qc::plant_model_variant(model)], blocks, qc::PLANT_BLOCK, stream, (long)n, a, qc::plant_model_args(model));
}

int qc_leg_plant_step_model_batch(qc_handle* h, size_t n, const qc_leg_plant_io* io, const qc_plant_model* model, void* stream) {
  if (const int rc = qc::check_leg_plant_model_args(h, n, io, model); rc != QC_OK || n == 0) return rc;
  qc::LegPlantArgs a;
  if (const int rc = qc::leg_plant_model_constants(h->dp.mass, h->dp.Ib, io, model, a); rc != QC_OK) return rc;
  QC_HIP(hipSetDevice(h->device));
  static void (*const kernels[8])(const qc::DevParams*, long, qc::LegPlantArgs, qc::PlantModelArgs) = QC_MODEL_KERNELS(leg_plant_step_model_kernel);
  const unsigned blocks = (unsigned)((n + qc::LEG_PLANT_BLOCK - 1) / qc::LEG_PLANT_BLOCK);
  return launch_flat(kernels[qc::plant_model_variant(model)], blocks, qc::LEG_PLANT_BLOCK, stream, h->d_params, (long)n, a, qc::plant_model_args(model));
}

int qc_plant_step_model_adjoint_batch(qc_handle* h, size_t n, const qc_plant_adjoint_io* io, const qc_plant_model* model,
                                      const qc_plant_model_bar* bar, void* stream) {
  if (const int rc = qc::check_plant_model_adjoint_args(h, n, io, model, bar); rc != QC_OK || n == 0) return rc;
  qc::PlantAdjointArgs a;
  if (const int rc = qc::plant_model_adjoint_constants(h->dp.mass, h->dp.Ib, io, model, a); rc != QC_OK) return rc;
  QC_HIP(hipSetDevice(h->device));
  static void (*const kernels[8])(long, qc::PlantAdjointArgs, qc::PlantModelArgs, qc::PlantModelBarArgs) = QC_MODEL_KERNELS(plant_step_model_adjoint_kernel);
  const unsigned blocks = (unsigned)((n + qc::PLANT_BLOCK - 1) / qc::PLANT_BLOCK);
  return launch_flat(kernels[qc::plant_model_variant(model)], blocks, qc::PLANT_BLOCK, stream, (long)n, a, qc::plant_model_args(model),
                     qc::plant_model_bar_args(bar));
}
#undef QC_MODEL_KERNELS

void qc_default_certify(qc_certify_io* io) {
  if (!zeroed(io)) return;
  io->act_tol = 1e-7;  // the defaults of tests/kkt_batch.py: kkt_batch's act_tol, assert_kkt's bars
  io->primal_tol = 1e-7;
  io->stat_tol = 1e-8;
}

int qc_certify_batch(qc_handle* h, size_t n, const qc_batch_in* in, const qc_certify_io* io, void* stream) {
  if (const int rc = qc::check_certify_args(h, n, in, io); rc != QC_OK || n == 0) return rc;
  QC_HIP(hipSetDevice(h->device));
  qc::CertifyArgs a{io->grf_body, io->act_tol, io->primal_tol, io->stat_tol, io->primal, io->stationarity, io->lambda, io->grad,
                    io->active, io->flags, io->summary ? h->certify_parts : nullptr};
  const unsigned blocks = qc::certify_blocks(n);
  if (const int rc = launch_per_robot(qc::certify_kernel<true>, qc::certify_kernel<false>, blocks, qc::CERTIFY_BLOCK, h, n, readonly_view(in, true), a, stream); rc != QC_OK) return rc;
  if (!io->summary) return QC_OK;
  return launch_flat(qc::certify_summary_kernel, 1, qc::CERTIFY_SUMMARY_BLOCK, stream, h->certify_parts, (int)blocks, reinterpret_cast<qc::CertifySummary*>(io->summary));
}

void qc_default_sensitivity(qc_sensitivity_io* io) {
  if (!zeroed(io)) return;
  io->act_tol = 1e-7;  // qc_default_certify's
}

int qc_sensitivity_batch(qc_handle* h, size_t n, const qc_batch_in* in, const qc_sensitivity_io* io, void* stream) {
  if (const int rc = qc::check_sensitivity_args(h, n, in, io); rc != QC_OK || n == 0) return rc;
  QC_HIP(hipSetDevice(h->device));
  qc::SensitivityArgs a{io->grf_body, io->grf_bar, io->act_tol, io->adjoint, io->b_bar, io->feet_bar, io->x_bar, io->xdot_bar, io->w_bar,
                        io->x_d_bar, io->xdot_d_bar, io->w_d_bar, io->flags};
  return launch_per_robot(qc::sensitivity_kernel<true>, qc::sensitivity_kernel<false>, qc::sensitivity_blocks(n), qc::SENSITIVITY_BLOCK, h, n, readonly_view(in, true), a, stream);
}

void qc_default_tangent(qc_tangent_io* io) {
  if (!zeroed(io)) return;
  io->act_tol = 1e-7;  // qc_default_sensitivity's
  io->n_dir = 1;
}

int qc_tangent_batch(qc_handle* h, size_t n, const qc_batch_in* in, const qc_tangent_io* io, void* stream) {
  if (const int rc = qc::check_tangent_args(h, n, in, io); rc != QC_OK || n == 0) return rc;
  QC_HIP(hipSetDevice(h->device));
  return launch_per_robot(qc::tangent_kernel<true>, qc::tangent_kernel<false>, qc::tangent_blocks(n), qc::TANGENT_BLOCK, h, n, readonly_view(in, true),
                          qc::tangent_constants(io), stream);
}

void qc_default_plant_tangent(qc_plant_tangent_io* io) {
  if (!zeroed(io)) return;
  io->dt = 1.0 / 300.0;  // qc_default_plant's
  io->n_dir = 1;
}

int qc_plant_step_tangent_batch(qc_handle* h, size_t n, const qc_plant_tangent_io* io, void* stream) {
  if (const int rc = qc::check_plant_tangent_args(h, n, io); rc != QC_OK || n == 0) return rc;
  qc::PlantTangentArgs a;
  if (const int rc = qc::plant_tangent_constants(h->dp.mass, h->dp.Ib, io, a); rc != QC_OK) return rc;
  QC_HIP(hipSetDevice(h->device));
  return launch_flat(qc::plant_step_tangent_kernel, qc::plant_tangent_blocks(n, io->n_dir), qc::PLANT_TANGENT_BLOCK, stream, (long)n, a);
}

void qc_default_torque_tangent(qc_torque_tangent_io* io) {
  if (!zeroed(io)) return;
  io->n_dir = 1;
}

int qc_torque_tangent_batch(qc_handle* h, size_t n, const qc_batch_in* in, const qc_torque_tangent_io* io, void* stream) {
  if (const int rc = qc::check_torque_tangent_args(h, n, in, io); rc != QC_OK || n == 0) return rc;
  QC_HIP(hipSetDevice(h->device));
  // (of `in`: joint_q and the contact mask as it is now - no state array, nothing that advances or plans)
  return launch_flat(qc::torque_tangent_kernel, qc::torque_tangent_blocks(n, io->n_dir), qc::TORQUE_TANGENT_BLOCK, stream, h->d_params, (long)(4 * n),
                     qc::torque_tangent_constants(in, io));
}

void qc_default_swing_tangent(qc_swing_tangent_io* io) {
  if (!zeroed(io)) return;
  io->n_dir = 1;
}

int qc_swing_torque_tangent_batch(qc_handle* h, size_t n, const qc_batch_in* in, const qc_swing_tangent_io* io, void* stream) {
  if (const int rc = qc::check_swing_tangent_args(h, n, in, io); rc != QC_OK || n == 0) return rc;
  QC_HIP(hipSetDevice(h->device));
  // (of `in`: the six arrays of the swing chain and the contact mask as it is now - nothing that advances or plans)
  return launch_flat(qc::swing_tangent_kernel, qc::swing_tangent_blocks(n, qc::swing_tangent_dirs(io)), qc::SWING_TANGENT_BLOCK, stream, h->d_params,
                     (long)(4 * n), qc::swing_tangent_constants(in, io));
}

void qc_default_leg_plant_tangent(qc_leg_plant_tangent_io* io) {
  if (!zeroed(io)) return;  // (leg_inertia 0, as qc_default_leg_plant leaves it)
  io->dt = 1.0 / 300.0;  // qc_default_leg_plant's
  io->n_dir = 1;
}

int qc_leg_plant_step_tangent_batch(qc_handle* h, size_t n, const qc_leg_plant_tangent_io* io, void* stream) {
  if (const int rc = qc::check_leg_plant_tangent_args(h, n, io); rc != QC_OK || n == 0) return rc;
  qc::LegPlantTangentArgs a;
  if (const int rc = qc::leg_plant_tangent_constants(h->dp.mass, h->dp.Ib, io, a); rc != QC_OK) return rc;
  QC_HIP(hipSetDevice(h->device));
  return launch_flat(qc::leg_plant_step_tangent_kernel, qc::leg_plant_tangent_blocks(n, io->n_dir), qc::LEG_PLANT_TANGENT_BLOCK, stream, h->d_params, (long)n, a);
}

void qc_default_swing_reference_tangent(qc_swing_reference_tangent_io* io) {
  if (!zeroed(io)) return;
  io->n_dir = 1;
}

int qc_swing_reference_tangent_batch(qc_handle* h, size_t n, const qc_batch_in* in, const qc_swing_reference_tangent_io* io, void* stream) {
  if (const int rc = qc::check_swing_reference_tangent_args(h, n, in, io); rc != QC_OK || n == 0) return rc;
  QC_HIP(hipSetDevice(h->device));
  // (of `in`: the state, joint_q and the contact mask as the forward call left it - nothing of it is written)
  return launch_flat(qc::swing_reference_tangent_kernel, qc::swing_reference_tangent_blocks(n, qc::swing_reference_tangent_dirs(io)),
                     qc::SWING_REFERENCE_TANGENT_BLOCK, stream, h->d_params, (long)n, qc::swing_reference_tangent_constants(in, io));
}

void qc_default_commander_step_tangent(qc_commander_step_tangent_io* io) {
  if (!zeroed(io)) return;
  io->n_dir = 1;
}

int qc_commander_step_tangent_batch(qc_handle* h, size_t n, const qc_batch_in* in, const qc_command_in* cmd, const qc_commander_step_tangent_io* io,
                                    void* stream) {
  if (const int rc = qc::check_commander_step_tangent_args(h, n, in, cmd, io); rc != QC_OK || n == 0) return rc;
  QC_HIP(hipSetDevice(h->device));
  // (cmd->state is not read: the records are io->state_before)
  return launch_flat(qc::commander_step_tangent_kernel, qc::command_tangent_blocks(n, qc::commander_step_tangent_dirs(io)), qc::COMMAND_TANGENT_BLOCK,
                     stream, (long)n, qc::commander_step_tangent_constants(in, cmd, io));
}

void qc_default_com_reference_tangent(qc_com_reference_tangent_io* io) {
  if (!zeroed(io)) return;
  io->mode = QC_COM_REPLACE;
  io->gain = 1.0;
  io->n_dir = 1;
}

int qc_com_reference_tangent_batch(qc_handle* h, size_t n, const qc_batch_in* in, const qc_com_reference_tangent_io* io, void* stream) {
  if (const int rc = qc::check_com_reference_tangent_args(h, n, in, io); rc != QC_OK || n == 0) return rc;
  QC_HIP(hipSetDevice(h->device));
  return launch_flat(qc::com_reference_tangent_kernel, qc::command_tangent_blocks(n, qc::com_reference_tangent_dirs(io)), qc::COMMAND_TANGENT_BLOCK,
                     stream, h->d_params, (long)n, qc::com_reference_tangent_constants(in, io));
}

void qc_default_param_tangent(qc_param_tangent_io* io) {
  if (!zeroed(io)) return;
  io->act_tol = 1e-7;  // qc_default_tangent's
  io->n_dir = 1;
}

int qc_param_tangent_batch(qc_handle* h, size_t n, const qc_batch_in* in, const qc_param_tangent_io* io, void* stream) {
  if (const int rc = qc::check_param_tangent_args(h, n, in, io); rc != QC_OK || n == 0) return rc;
  QC_HIP(hipSetDevice(h->device));
  return launch_per_robot(qc::param_tangent_kernel<true>, qc::param_tangent_kernel<false>, qc::param_tangent_blocks(n), qc::PARAM_TANGENT_BLOCK, h, n,
                          readonly_view(in, true), qc::param_tangent_constants(io), stream);
}

void qc_default_sensitivity_rot(qc_sensitivity_rot_io* io) { (void)zeroed(io); }

int qc_sensitivity_rot_batch(qc_handle* h, size_t n, const qc_batch_in* in, const qc_sensitivity_rot_io* io, void* stream) {
  if (const int rc = qc::check_sensitivity_rot_args(h, n, in, io); rc != QC_OK || n == 0) return rc;
  QC_HIP(hipSetDevice(h->device));
  qc::SensitivityRotArgs a{io->grf_body, io->grf_bar, io->b_bar, io->feet_bar, io->Rwb_bar, io->Rwb_d_bar, io->Rwb_rot_bar, io->Rwb_d_rot_bar};
  // (no contact mask: swing feet carry zeros)
  return launch_per_robot(qc::sensitivity_rot_kernel<true>, qc::sensitivity_rot_kernel<false>, qc::sensitivity_blocks(n), qc::SENSITIVITY_BLOCK, h, n, readonly_view(in, false), a, stream);
}

void qc_default_sensitivity_param(qc_sensitivity_param_io* io) {
  if (!zeroed(io)) return;
  io->act_tol = 1e-7;  // qc_default_sensitivity's
}

int qc_sensitivity_param_batch(qc_handle* h, size_t n, const qc_batch_in* in, const qc_sensitivity_param_io* io, void* stream) {
  if (const int rc = qc::check_sensitivity_param_args(h, n, in, io); rc != QC_OK || n == 0) return rc;
  QC_HIP(hipSetDevice(h->device));
  qc::SensitivityParamArgs a{io->grf_body, io->grf_bar, io->adjoint, io->act_tol, io->param_bar_rows, io->param_bar ? h->param_parts : nullptr};
  const unsigned blocks = qc::sensitivity_param_blocks(n);
  if (const int rc = launch_per_robot(qc::sensitivity_param_kernel<true>, qc::sensitivity_param_kernel<false>, blocks, qc::SENSITIVITY_PARAM_BLOCK, h, n, readonly_view(in, true), a, stream); rc != QC_OK) return rc;
  if (!io->param_bar) return QC_OK;
  return launch_flat(qc::sensitivity_param_sum_kernel, 1, qc::SENSITIVITY_PARAM_SUM_BLOCK, stream, h->param_parts, (int)blocks, io->param_bar);
}

void qc_default_sensitivity_kin(qc_sensitivity_kin_io* io) { (void)zeroed(io); }

int qc_sensitivity_kin_batch(qc_handle* h, size_t n, const qc_batch_in* in, const qc_sensitivity_kin_io* io, void* stream) {
  if (const int rc = qc::check_sensitivity_kin_args(h, n, in, io); rc != QC_OK || n == 0) return rc;
  QC_HIP(hipSetDevice(h->device));
  // (of `in`: joint_q and the contact mask as it is now - no state array, nothing that advances or plans)
  const qc::SensitivityKinArgs a{in->joint_q, in->stance, in->gait_phase, in->gait_duty, io->grf_body, io->status, io->joint_tau_bar, io->feet_bar,
                                 io->grf_bar_in, io->joint_q_bar_in, io->grf_bar, io->joint_q_bar};
  const bool tau = io->joint_tau_bar != nullptr, fk = io->feet_bar != nullptr;
  const auto fn = pick2(tau, fk, qc::sensitivity_kin_kernel<true, true>, qc::sensitivity_kin_kernel<true, false>, qc::sensitivity_kin_kernel<false, true>,
                        qc::sensitivity_kin_kernel<false, false>);
  return launch_flat(fn, qc::sensitivity_kin_blocks(n), qc::SENSITIVITY_BLOCK, stream, h->d_params, (long)(4 * n), a);
}

void qc_default_sensitivity_swing(qc_sensitivity_swing_io* io) { (void)zeroed(io); }

int qc_sensitivity_swing_batch(qc_handle* h, size_t n, const qc_batch_in* in, const qc_sensitivity_swing_io* io, void* stream) {
  if (const int rc = qc::check_sensitivity_swing_args(h, n, in, io); rc != QC_OK || n == 0) return rc;
  QC_HIP(hipSetDevice(h->device));
  // (of `in`: the six arrays of the swing chain and the contact mask as it is now - nothing that advances or plans)
  const qc::SensitivitySwingArgs a{in->Rwb, in->x, in->joint_q, in->joint_qdot, in->swing_pos, in->swing_vel, in->stance, in->gait_phase, in->gait_duty,
                                   io->joint_tau_bar, io->joint_q_bar_in, io->Rwb_bar_in, io->x_bar_in, io->swing_pos_bar, io->swing_vel_bar,
                                   io->joint_q_bar, io->joint_qdot_bar, io->gain_bar, io->Rwb_bar, io->x_bar, io->flags};
  const bool leg = io->swing_pos_bar || io->swing_vel_bar || io->joint_q_bar || io->joint_qdot_bar || io->gain_bar, body = io->Rwb_bar || io->x_bar;
  const auto fn = pick2(leg, body, qc::sensitivity_swing_kernel<true, true>, qc::sensitivity_swing_kernel<true, false>,
                        qc::sensitivity_swing_kernel<false, true>, qc::sensitivity_swing_kernel<false, false>);
  return launch_flat(fn, qc::sensitivity_swing_blocks(n), qc::SENSITIVITY_BLOCK, stream, h->d_params, (long)(4 * n), a);
}

void qc_default_swing_reference(qc_swing_reference_io* io) { (void)zeroed(io); }

int qc_swing_reference_batch(qc_handle* h, size_t n, const qc_batch_in* in, const qc_swing_reference_io* io, void* stream) {
  if (const int rc = qc::check_swing_reference_args(h, n, in, io); rc != QC_OK || n == 0) return rc;
  QC_HIP(hipSetDevice(h->device));
  const qc::SwingReferenceArgs a{in->Rwb, in->x, in->xdot, in->w, in->xdot_d, in->joint_q, in->gait_phase, in->stance, in->gait_duty, in->gait_dt,
                                 reinterpret_cast<qc::SwingState*>(in->swing_state), io->swing_pos, io->swing_vel, io->planned};
  return launch_flat(qc::swing_reference_kernel, qc::swing_reference_blocks(n), qc::SENSITIVITY_BLOCK, stream, h->d_params, (long)n, a);
}

void qc_default_swing_reference_adjoint(qc_swing_reference_adjoint_io* io) { (void)zeroed(io); }

int qc_swing_reference_adjoint_batch(qc_handle* h, size_t n, const qc_batch_in* in, const qc_swing_reference_adjoint_io* io, void* stream) {
  if (const int rc = qc::check_swing_reference_adjoint_args(h, n, in, io); rc != QC_OK || n == 0) return rc;
  QC_HIP(hipSetDevice(h->device));
  // (of `in`: the state, joint_q and the contact mask as the forward call left it - nothing of it is written)
  const qc::SwingReferenceAdjointArgs a{in->Rwb, in->x, in->xdot, in->w, in->joint_q, in->gait_phase, in->stance, in->gait_duty,
                                        reinterpret_cast<const qc::SwingState*>(io->state_before), io->swing_pos_bar, io->swing_vel_bar,
                                        io->p_start_next_bar, io->p_final_next_bar, io->Rwb_bar_in, io->x_bar_in, io->xdot_bar_in, io->w_bar_in,
                                        io->joint_q_bar_in, io->Rwb_bar, io->x_bar, io->xdot_bar, io->w_bar, io->xdot_d_bar, io->joint_q_bar,
                                        io->p_start_bar, io->p_final_bar, io->flags};
  return launch_flat(qc::swing_reference_adjoint_kernel, qc::swing_reference_blocks(n), qc::SENSITIVITY_BLOCK, stream, h->d_params, (long)n, a);
}

void qc_default_commander_step(qc_commander_step_io* io) { (void)zeroed(io); }

int qc_commander_step_batch(qc_handle* h, size_t n, const qc_batch_in* in, const qc_command_in* cmd, const qc_commander_step_io* io, void* stream) {
  if (const int rc = qc::check_commander_step_args(h, n, in, cmd, io); rc != QC_OK || n == 0) return rc;
  QC_HIP(hipSetDevice(h->device));
  const qc::CommanderStepArgs a{in->Rwb, in->x, cmd->twist, cmd->fresh, reinterpret_cast<qc::CmdState*>(cmd->state), cmd->stand_height, cmd->stand_tol,
                                cmd->cmd_dt, io->Rwb_d, io->x_d, io->xdot_d, io->w_d, io->run, io->applied};
  return launch_flat(qc::commander_step_kernel, qc::commander_step_blocks(n), qc::SENSITIVITY_BLOCK, stream, (long)n, a);
}

void qc_default_commander_step_adjoint(qc_commander_step_adjoint_io* io) { (void)zeroed(io); }

int qc_commander_step_adjoint_batch(qc_handle* h, size_t n, const qc_batch_in* in, const qc_command_in* cmd, const qc_commander_step_adjoint_io* io,
                                    void* stream) {
  if (const int rc = qc::check_commander_step_adjoint_args(h, n, in, cmd, io); rc != QC_OK || n == 0) return rc;
  QC_HIP(hipSetDevice(h->device));
  // (of `cmd`: twist, fresh and the three scalars - its records are not read, the ones from before the forward call are)
  const qc::CommanderStepAdjointArgs a{in->Rwb, in->x, cmd->twist, cmd->fresh, reinterpret_cast<const qc::CmdState*>(io->state_before), cmd->stand_height,
                                       cmd->stand_tol, cmd->cmd_dt, io->Rwb_d_bar, io->x_d_bar, io->xdot_d_bar, io->w_d_bar, io->Vb_next_bar,
                                       io->Rwb_bar_in, io->x_bar_in, io->twist_bar, io->Vb_bar, io->Rwb_bar, io->x_bar, io->Rwb_d_prev_bar,
                                       io->x_d_prev_bar, io->xdot_d_prev_bar, io->w_d_prev_bar, io->flags};
  return launch_flat(qc::commander_step_adjoint_kernel, qc::commander_step_blocks(n), qc::SENSITIVITY_BLOCK, stream, (long)n, a);
}

void qc_default_support_polygon(qc_support_polygon_io* io) { (void)zeroed(io); }

int qc_support_polygon_batch(qc_handle* h, size_t n, const qc_batch_in* in, const qc_support_polygon_io* io, void* stream) {
  if (const int rc = qc::check_support_polygon_args(h, n, in, io); rc != QC_OK || n == 0) return rc;
  QC_HIP(hipSetDevice(h->device));
  // (of `in`: the feet, the phases and the contact mask as it is now, the pose in world mode - nothing of it is written)
  const qc::SupportPolygonArgs a{qc::support_in(in, io->schedule, io->schedule_shared, io->world != 0), io->com_xy, io->weights, io->flags};
  return launch_flat(qc::support_polygon_kernel, qc::support_polygon_blocks(n), qc::SENSITIVITY_BLOCK, stream, h->d_params, (long)n, a);
}

void qc_default_support_polygon_adjoint(qc_support_polygon_adjoint_io* io) { (void)zeroed(io); }

int qc_support_polygon_adjoint_batch(qc_handle* h, size_t n, const qc_batch_in* in, const qc_support_polygon_adjoint_io* io, void* stream) {
  if (const int rc = qc::check_support_polygon_adjoint_args(h, n, in, io); rc != QC_OK || n == 0) return rc;
  QC_HIP(hipSetDevice(h->device));
  const qc::SupportPolygonAdjointArgs a{qc::support_in(in, io->schedule, io->schedule_shared, io->world != 0), io->com_xy_bar, io->feet_bar_in,
                                        io->Rwb_bar_in, io->x_bar_in, io->phase_bar_in, io->schedule_bar_in, io->feet_bar, io->Rwb_bar, io->x_bar,
                                        io->phase_bar, io->schedule_bar, io->flags};
  return launch_flat(qc::support_polygon_adjoint_kernel, qc::support_polygon_blocks(n), qc::SENSITIVITY_BLOCK, stream, h->d_params, (long)n, a);
}

void qc_default_com_reference(qc_com_reference_io* io) {
  if (!zeroed(io)) return;
  io->mode = QC_COM_REPLACE;
  io->gain = 1.0;
}

int qc_com_reference_batch(qc_handle* h, size_t n, const qc_batch_in* in, const qc_com_reference_io* io, void* stream) {
  if (const int rc = qc::check_com_reference_args(h, n, in, io); rc != QC_OK || n == 0) return rc;
  QC_HIP(hipSetDevice(h->device));
  // (of `in`: the feet, the phases and the contact mask as it is now, the pose - nothing of it is written)
  const qc::ComReferenceArgs a{qc::support_in(in, io->schedule, io->schedule_shared, true), io->x_d_in, io->mode, io->gain, io->x_d_out, io->com_xy, io->flags};
  return launch_flat(qc::com_reference_kernel, qc::com_reference_blocks(n, false), qc::SENSITIVITY_BLOCK, stream, h->d_params, (long)n, a);
}

void qc_default_com_reference_adjoint(qc_com_reference_adjoint_io* io) {
  if (!zeroed(io)) return;
  io->mode = QC_COM_REPLACE;
  io->gain = 1.0;
}

int qc_com_reference_adjoint_batch(qc_handle* h, size_t n, const qc_batch_in* in, const qc_com_reference_adjoint_io* io, void* stream) {
  if (const int rc = qc::check_com_reference_adjoint_args(h, n, in, io); rc != QC_OK || n == 0) return rc;
  QC_HIP(hipSetDevice(h->device));
  const bool sum = io->schedule_bar_sum != nullptr;
  const qc::SupportIn s = qc::support_in(in, io->schedule, io->schedule_shared, true);
  const qc::ComReferenceAdjointArgs a{s.feet, s.joint_q, s.gait_phase, s.stance, s.gait_duty, s.Rwb, s.x, s.schedule, s.shared, io->mode, io->gain,
                                      io->x_d_out_bar, io->feet_bar_in, io->Rwb_bar_in, io->x_bar_in, io->phase_bar_in, io->schedule_bar_in, io->x_d_in_bar,
                                      io->feet_bar, io->Rwb_bar, io->x_bar, io->phase_bar, io->schedule_bar, sum ? h->com_parts : nullptr, io->flags};
  const unsigned blocks = qc::com_reference_blocks(n, sum);
  if (sum) {
    if (const int rc = launch_flat(qc::com_reference_adjoint_kernel<true>, blocks, qc::SENSITIVITY_BLOCK, stream, h->d_params, (long)n, a); rc != QC_OK) return rc;
    return launch_flat(qc::com_schedule_sum_kernel, 1, qc::COM_SUM_FINISH_BLOCK, stream, h->com_parts, (int)blocks, io->schedule_bar_sum);
  }
  return launch_flat(qc::com_reference_adjoint_kernel<false>, blocks, qc::SENSITIVITY_BLOCK, stream, h->d_params, (long)n, a);
}

// host-pointer variant.  Large batches: one device staging allocation, H2D copies, kernel, D2H copies, sync.
// Small batches (n <= kPinnedMaxN; the reference's own use is one robot per controller tick): the records are packed
// into a pinned, device-visible host buffer that the kernel reads and writes in place over PCIe - one launch and one
// stream synchronise instead of a dozen staged copies.
static constexpr size_t kPinnedMaxN = 8192;  // measured crossover with the staged copies: ~16 384 robots (config 2 records)
int qc_control_batch_host(qc_handle* h, size_t n, const qc_batch_in* in, const uint32_t* warm, const qc_batch_out* out) {
  if (const int rc = qc::check_batch_args("qc_control_batch_host", h, n, in, out, false); rc != QC_OK || n == 0) return rc;
  QC_HIP(hipSetDevice(h->device));
  if (!h->stream) QC_HIP(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
  const bool pinned = n <= kPinnedMaxN;
  // layout (all 16-byte aligned slices): 48 doubles in, 12 doubles out, 4 x 4-byte words, optional arrays
  const size_t per = 48 * 8 + 12 * 8 + 4 * 4 + 8 + 12 * 8 + 12 * 8 + 6 * 8 + 3 * 12 * 8 + sizeof(qc_swing_state);
  const size_t need = n * per + 512;
  char* base;
  if (pinned) {
    if (need > h->pin_bytes) {  // grows on demand: a handle that only ever sees one robot per call keeps ~2 KB pinned
      if (h->pin) QC_HIP(hipHostFree(h->pin));
      h->pin = nullptr; h->pin_bytes = 0;
      QC_HIP(hipHostMalloc(&h->pin, need, hipHostMallocDefault));
      h->pin_bytes = need;
    }
    base = (char*)h->pin;
  } else {
    if (need > h->stage_bytes) {
      if (h->stage) QC_HIP(hipFree(h->stage));
      h->stage = nullptr; h->stage_bytes = 0;
      QC_HIP(hipMalloc(&h->stage, need));
      h->stage_bytes = need;
    }
    base = (char*)h->stage;
  }
  size_t off = 0;
  auto carve = [&](size_t bytes) { char* p = base + off; off += (bytes + 15) & ~(size_t)15; return p; };
  hipError_t cerr = hipSuccess;
  auto put = [&](const void* src, size_t bytes) -> void* {  // input slice: carve + host -> buffer
    if (!src) return nullptr;
    char* d = carve(bytes);
    if (pinned) std::memcpy(d, src, bytes);
    else if (cerr == hipSuccess) cerr = hipMemcpyAsync(d, src, bytes, hipMemcpyHostToDevice, h->stream);
    return d;
  };
  auto get = [&](void* dst, const void* d, size_t bytes) {  // output slice: buffer -> host
    if (!dst || !d) return;
    if (pinned) std::memcpy(dst, d, bytes);
    else if (cerr == hipSuccess) cerr = hipMemcpyAsync(dst, d, bytes, hipMemcpyDeviceToHost, h->stream);
  };
  qc_batch_in din{};
  din.Rwb = (const double*)put(in->Rwb, n * 9 * 8);
  din.Rwb_d = (const double*)put(in->Rwb_d, n * 9 * 8);
  din.x = (const double*)put(in->x, n * 3 * 8);
  din.xdot = (const double*)put(in->xdot, n * 3 * 8);
  din.w = (const double*)put(in->w, n * 3 * 8);
  din.x_d = (const double*)put(in->x_d, n * 3 * 8);
  din.xdot_d = (const double*)put(in->xdot_d, n * 3 * 8);
  din.w_d = (const double*)put(in->w_d, n * 3 * 8);
  din.feet = (const double*)put(in->feet, n * 12 * 8);  // may be absent when joint_q is given
  din.stance = (const uint8_t*)put(in->stance, n * 4);
  din.joint_q = (const double*)put(in->joint_q, n * 12 * 8);
  din.gait_phase = (double*)put(in->gait_phase, n * 4 * 8);
  din.gait_duty = (const double*)put(in->gait_duty, n * 8);
  din.gait_dt = (const double*)put(in->gait_dt, n * 8);
  din.swing_pos = (const double*)put(in->swing_pos, n * 12 * 8);
  din.swing_vel = (const double*)put(in->swing_vel, n * 12 * 8);
  din.joint_qdot = (const double*)put(in->joint_qdot, n * 12 * 8);
  din.swing_state = (qc_swing_state*)put(in->swing_state, n * sizeof(qc_swing_state));  // in/out
  const uint32_t* d_warm = (const uint32_t*)put(warm, n * 4);
  qc_batch_out dout{};
  dout.grf_body = (double*)carve(n * 12 * 8);
  dout.status = (int32_t*)carve(n * 4);
  dout.active_set = out->active_set ? (uint32_t*)carve(n * 4) : nullptr;
  dout.iterations = out->iterations ? (int32_t*)carve(n * 4) : nullptr;
  dout.joint_tau = out->joint_tau ? (double*)carve(n * 12 * 8) : nullptr;
  QC_HIP(cerr);
  if (off > (pinned ? h->pin_bytes : h->stage_bytes)) return fail(QC_ERR_INVALID, "qc_control_batch_host: staging overflow");
  int rc = qc_control_batch(h, n, &din, d_warm, &dout, h->stream);
  if (rc != QC_OK) return rc;
  if (pinned) QC_HIP(hipStreamSynchronize(h->stream));  // kernel-end release makes the in-place results visible
  get(out->grf_body, dout.grf_body, n * 12 * 8);
  get(out->status, dout.status, n * 4);
  get(out->active_set, dout.active_set, n * 4);
  get(out->iterations, dout.iterations, n * 4);
  get(out->joint_tau, dout.joint_tau, n * 12 * 8);
  get(in->swing_state, din.swing_state, n * sizeof(qc_swing_state));
  if (in->gait_dt) get(in->gait_phase, din.gait_phase, n * 4 * 8);  // the advanced clock
  QC_HIP(cerr);
  if (!pinned) QC_HIP(hipStreamSynchronize(h->stream));
  return QC_OK;
}

int qc_control(qc_handle* h, const double* Rwb, const double* Rwb_d, const double* x, const double* xdot,
               const double* w, const double* x_d, const double* xdot_d, const double* w_d, const double* feet,
               const uint8_t* stance, double* grf_body, int32_t* status) {
  if (!h || !status) return fail(QC_ERR_INVALID, "qc_control: null argument");
  qc_batch_in in{Rwb, Rwb_d, x, xdot, w, x_d, xdot_d, w_d, feet, stance, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  // The handle remembers the working set of its previous call and starts from it - the per-instance hot-start
  // memory of the reference's SQProblem (BC.hpp:161, BC.cpp:191-202).  Same minimiser either way (strictly convex).
  uint32_t word_in = h->last_word, word_out = 0;
  qc_batch_out out{grf_body, status, &word_out, nullptr, nullptr};
  const int rc = qc_control_batch_host(h, 1, &in, h->has_last ? &word_in : nullptr, &out);
  h->has_last = rc == QC_OK && *status == QC_SOLVED;
  h->last_word = word_out;
  return rc;
}

}  // extern "C"
