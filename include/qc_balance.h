/* qc_balance.h - C ABI of the MI355X-native batched balance controller.
 *
 * Drop-in boundary for ONE path of bostoncleek/quadruped_control:
 *   quadruped_controller::BalanceController::control()
 *     quadruped_controller/include/quadruped_controller/balance_controller.hpp:85-107
 *     quadruped_controller/src/quadruped_controller/balance_controller.cpp:70-330
 * i.e. PD wrench law -> single-rigid-body Newton-Euler map -> 12-variable
 * friction-cone QP (solved there by qpOASES SQProblem, balance_controller.cpp:177-210)
 * -> body-frame ground reaction forces.  One *instance* = one robot tick; the
 * batch axis is "independent robots".  All arithmetic is FP64, leg order is
 * RL, FL, RR, FR (commander_node.cpp:61), matrices are row-major.
 *
 * Plain C: pointers and sizes only, no C++/torch types, no exceptions.
 * The library is HIP-only (gfx950); there is no CPU fallback behind this ABI.
 */
#ifndef QC_BALANCE_H
#define QC_BALANCE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QC_ABI_VERSION 6
#define QC_PARAM_COUNT 211 /* the doubles of qc_params, in its order: the layout of a parameter cotangent (qc_sensitivity_param_batch) */

/* Replaces the constructor arguments of BalanceController
 * (balance_controller.hpp:85-88; defaults in commander_node.cpp:289-334 and
 * quadruped_simulation/config/mit_cheetah_config.yaml:66-99). */
typedef struct qc_params {
  double mu;       /* friction coefficient                                  */
  double mass;     /* total mass (kg)                                       */
  double fzmin;    /* min normal force (N), 0 <= fzmin <= fzmax             */
  double fzmax;    /* max normal force (N)                                  */
  double Ib[9];    /* trunk inertia, body frame (3x3)                       */
  double S[36];    /* SPD weight on the wrench residual (6x6)               */
  double W[144];   /* SPD weight on the forces (12x12)                      */
  double kff[6];   /* feed-forward gains                                    */
  double kp_p[3];  /* COM position Kp                                       */
  double kd_p[3];  /* COM linear-velocity Kd                                */
  double kp_w[3];  /* COM orientation Kp                                    */
  double kd_w[3];  /* COM angular-velocity Kd                               */
  int32_t max_iter; /* working-set recalculation cap; <=0 -> 200 (nWSR_, balance_controller.cpp:85); at most QC_MAX_ITER_LIMIT */
  int32_t reserved;
} qc_params;

/* Replaces the per-call arguments of control() (balance_controller.hpp:104-107),
 * one row per robot.  DEVICE pointers for qc_control_batch, HOST pointers for
 * qc_control_batch_host.  8-byte aligned; `stance` may be NULL = make_stance_gait()
 * (gait.cpp:24-34, the default argument of control()). */
typedef struct qc_batch_in {
  const double* Rwb;     /* [n][9]  rotation world<-base                     */
  const double* Rwb_d;   /* [n][9]  desired rotation                         */
  const double* x;       /* [n][3]  COM position                             */
  const double* xdot;    /* [n][3]  COM linear velocity                      */
  const double* w;       /* [n][3]  COM angular velocity                     */
  const double* x_d;     /* [n][3]  desired COM position                     */
  const double* xdot_d;  /* [n][3]  desired COM linear velocity              */
  const double* w_d;     /* [n][3]  desired COM angular velocity             */
  const double* feet;    /* [n][4][3] foot positions, body frame (FootholdMap, types.hpp:108) */
  const uint8_t* stance; /* [n][4]  LegState per leg: 1 stance, 0 swing (GaitMap, types.hpp:91-100) */
  /* ABI v2, optional (NULL = unused).  Joint angles [n][4][3] (RL,FL,RR,FR x hip,thigh,calf; JointStatesMap,
   * types.hpp:127).  When given, the foot positions are computed on the device by the reference's forward
   * kinematics (kinematics.cpp:81-103, what commander_node.cpp:383-384 does before control()) and `feet`
   * is ignored (may be NULL). */
  const double* joint_q;
  /* ABI v2, optional.  Per-leg gait phases [n][4] in [0,1) (GaitScheduler::phases_, gait.cpp:113-123).
   * When given (and `stance` is NULL) the contact state is derived on the device by the reference's rule
   * (GaitScheduler::phase, gait.cpp:125-134): stance iff 0 <= phase <= stance_phase, each comparison with the
   * 1e-12 slack of math::almost_equal.  `gait_duty` [n] = stance_phase = t_stance / (t_swing + t_stance)
   * (gait.cpp:45) per robot, or NULL to use the value installed with qc_set_gait (default 0.8/0.98,
   * mit_cheetah_config.yaml:17-18). */
  double* gait_phase;   /* read-only unless gait_dt is given (then IN/OUT, see below) */
  const double* gait_duty;
  /* ABI v2, optional; all three or none, need joint_q and joint_tau.  Swing-leg references as the reference's
   * FootTrajectoryManager::referenceState() returns them (WORLD frame foot position / velocity, [n][4][3], read
   * for swing legs only) and the measured joint velocities [n][4][3].  The swing legs' entries of joint_tau
   * then hold the reference's swing-leg torque (commander_node.cpp:482-504, 514-526):
   *   p_b = Rwb^T pos - x (sic), v_b = Rwb^T vel, q_ref = legInverseKinematics(p_b) (kinematics.cpp:117-160),
   *   qdot_ref = legJacobianInverse(q_ref) v_b (kinematics.cpp:190-204),
   *   tau = kp o wrapPI(wrap2PI(q_ref) - wrap2PI(q)) + kd o (qdot_ref - qdot) + kff (joint_controller.cpp:21-39),
   * clamped like the stance torques; it does not depend on the QP's status. */
  const double* swing_pos;
  const double* swing_vel;
  const double* joint_qdot;
  /* ABI v2, optional, IN/OUT: persistent per-robot swing-planning state [n] (zero-initialise with
   * qc_swing_state_init before the first tick).  When given (needs joint_q, joint_qdot, gait_phase and
   * joint_tau; swing_pos/swing_vel must be NULL) the swing references are generated on the device the way
   * the reference's loop does it (commander_node.cpp:432-471): FootPlanner::positions / updateStates /
   * singleFoot (foot_planner.cpp:46-157: replan a foothold when a leg goes stance -> swing, Raibert + LIP
   * heuristic), FootTrajectoryManager::referenceStates / referenceState and the sextic FootTrajectory
   * (trajectory.cpp:220-277, 308-388), then fed to the swing-leg torque chain above. */
  struct qc_swing_state* swing_state;
  /* ABI v3, optional: the gait clock.  Time step [n] (seconds) since the robot's previous tick.  When given,
   * `gait_phase` is IN/OUT: at the start of the robot's tick its four phases advance the way
   * GaitScheduler::update does (gait.cpp:113-123): phase += 1 / (t_swing + t_stance) * dt, wrapped by
   * fmod(., 1), with the periods installed by qc_set_gait - and the contact rule, the foothold planner and
   * the swing trajectories of this tick see the advanced phases.  The buffer behind `gait_phase` is written
 * (which is why that member is not const). */
  const double* gait_dt;
} qc_batch_in;

/* FootPlanner::state_map_ (foot_planner.hpp) + FootTrajectoryManager::traj_map_ (trajectory.hpp), per robot. */
typedef struct qc_swing_state {
  int32_t leg_state[4];  /* LegState seen at the previous tick, -1 = none yet (state_map_ empty)     */
  int32_t has_traj[4];   /* leg has an entry in traj_map_                                            */
  double p_start[12];    /* [leg][xyz] world-frame trajectory start  (FootTrajBounds, types.hpp:52-66) */
  double p_final[12];    /* [leg][xyz] world-frame planned foothold                                   */
} qc_swing_state;

/* Replaces the returned ForceMap (types.hpp:119; balance_controller.cpp:218-232). */
typedef struct qc_batch_out {
  double* grf_body;     /* [n][4][3] = -Rwb^T f_world for stance legs; 0 for swing legs
                           (the reference omits swing legs from the map); 0 if status != 0 */
  int32_t* status;      /* [n] qc_status; != 0 is the reference's "empty ForceMap" (balance_controller.cpp:182-216) */
  uint32_t* active_set; /* [n] optional (may be NULL): optimal working set, feed back as `warm` next tick */
  int32_t* iterations;  /* [n] optional (may be NULL): working-set recalculations used */
  /* ABI v2, optional (NULL = unused; needs qc_batch_in.joint_q).  Stance-leg joint torques [n][4][3]:
   * tau = J(q_leg)^T f_body (QuadrupedKinematics::jacobianTransposeControl, kinematics.cpp:219-231 with
   * legJacobian :162-188), clamped to [tau_min, tau_max] as commander_node.cpp:523-526; failed instances get 0.
   * Swing legs get 0 as well unless swing references are given (qc_batch_in.swing_pos / swing_vel / joint_qdot, or
   * swing_state): then their entries hold the reference's swing-leg joint PD torque (commander_node.cpp:482-504),
   * whatever the QP's status. */
  double* joint_tau;
} qc_batch_out;

/* Kinematic constants of QuadrupedKinematics::QuadrupedKinematics() (kinematics.cpp:20-47) and the torque
 * limits of commander_node.cpp:324-325.  qc_create installs the reference's values. */
typedef struct qc_kinematics {
  double hip[12];   /* [leg][xyz] translation base -> hip   (trans_rl/fl/rr/fr)            */
  double links[12]; /* [leg][l1,l2,l3] signed link lengths  (left_links / right_links)     */
  double tau_min;   /* balance_control/torque_min (-20)                                     */
  double tau_max;   /* balance_control/torque_max (+20)                                     */
  double jc_kff[3]; /* joint_control/kff (0,0,0)      swing-leg joint PD, commander_node.cpp:314-341, */
  double jc_kp[3];  /* joint_control/kp  (40,40,50)   mit_cheetah_config.yaml:50-53                   */
  double jc_kd[3];  /* joint_control/kd  (1,1,1)                                                      */
  double planner_hip[12]; /* [leg][xyz] base -> thigh used by FootPlanner (foot_planner.cpp:27-42)          */
  double planner_k;       /* Raibert feedback gain k_ (foot_planner.cpp:25, 0.01)                            */
  double swing_height;    /* gait/height: apex of the swing trajectory (commander_node.cpp:247, 0.08)        */
} qc_kinematics;

typedef enum qc_status {
  QC_SOLVED = 0,
  QC_MAX_ITER = 1,   /* RET_MAX_NWSR_REACHED analogue */
  QC_INFEASIBLE = 2, /* kept for ABI completeness; cannot occur for 0 <= fzmin <= fzmax */
  QC_NOT_PD = 3      /* Hessian not positive definite / non-finite input (balance_controller.cpp:155-158 only logs) */
} qc_status;

/* return codes of the entry points */
#define QC_OK 0
#define QC_ERR_INVALID (-1) /* bad argument (see qc_last_error)  */
#define QC_ERR_HIP (-2)     /* HIP runtime error                 */
#define QC_ERR_NO_DEVICE (-3)
#define QC_ERR_ABI (-4)     /* caller and library were built against different revisions of this header */
#define QC_MAX_ITER_LIMIT 65535 /* largest recalculation cap (qc_params.max_iter, "max_iter" tuning key) */

typedef struct qc_handle qc_handle;

/* BalanceController::BalanceController (balance_controller.cpp:70-96).
 * `device` = HIP device ordinal.  A handle is used by one thread at a time
 * (like the reference object, whose control() mutates `mutable` members,
 * balance_controller.hpp:161-176); distinct handles are independent.
 *
 * ABI v6: the EXPORTED constructor is qc_create_abi, which also takes the caller's view of this header (QC_ABI_VERSION and
 * the sizes of the three structs that cross the boundary) and refuses a mismatch with QC_ERR_ABI before anything is read -
 * qc_batch_in has grown with every revision and carries no size field, so a caller built against an older header would
 * otherwise have its struct read past the end.  qc_create is the inline wrapper below: C and C++ callers keep writing
 * qc_create(&params, device, &handle) and cannot skip the guard; the library no longer exports a symbol of that name, so a
 * binary built against ABI <= 5 fails to link / load instead of running.  Bindings without a C compiler (ctypes, cgo, JNI)
 * call qc_create_abi with the sizes of THEIR mirror structs. */
int qc_create_abi(const qc_params* params, int device, qc_handle** out, int abi_version, size_t sizeof_params,
                  size_t sizeof_batch_in, size_t sizeof_batch_out);
void qc_destroy(qc_handle* h);

/* control() for n robots, device-resident inputs/outputs, asynchronous on
 * `stream` (a hipStream_t, NULL = default stream).  `warm` = device array [n]
 * of active_set words from the previous tick (the qpOASES hotstart analogue,
 * balance_controller.cpp:191-202) or NULL for a cold start. */
int qc_control_batch(qc_handle* h, size_t n, const qc_batch_in* in, const uint32_t* warm,
                     const qc_batch_out* out, void* stream);

/* Same with HOST pointers: stages through handle-owned device buffers and
 * synchronises before returning. */
int qc_control_batch_host(qc_handle* h, size_t n, const qc_batch_in* in, const uint32_t* warm,
                          const qc_batch_out* out);

/* One robot, host arguments laid out exactly like control()'s parameter list;
 * what the C++ BalanceController adapter (include/qc_balance_controller.hpp) calls.
 * Like the reference object (mutable SQProblem, balance_controller.hpp:161; init()/hotstart(),
 * balance_controller.cpp:177-202) the handle keeps the working set of its previous successful call
 * and starts the next one from it; the result is the same unique minimiser either way. */
int qc_control(qc_handle* h, const double* Rwb, const double* Rwb_d, const double* x,
               const double* xdot, const double* w, const double* x_d, const double* xdot_d,
               const double* w_d, const double* feet, const uint8_t* stance, double* grf_body,
               int32_t* status);

/* Kinematic model used by the joint_q / joint_tau extension; NULL restores the reference's constants.
 * qc_set_kinematics / qc_set_gait are configuration calls: they wait for all work on the device
 * (hipDeviceSynchronize) before rewriting the constants, so no launch in flight - on any stream - sees a
 * half-written copy. */
void qc_default_kinematics(qc_kinematics* out);
int qc_set_kinematics(qc_handle* h, const qc_kinematics* kin);
/* Default stance_phase for qc_batch_in.gait_phase: t_stance / (t_swing + t_stance), GaitScheduler ctor gait.cpp:36-46. */
int qc_set_gait(qc_handle* h, double t_swing, double t_stance);
/* Host helper: the "nothing planned yet" value of qc_swing_state for n robots (host memory). */
void qc_swing_state_init(struct qc_swing_state* states, size_t n);

/* Thread-local message of the last failing call (ROS_ERROR replacement,
 * balance_controller.cpp:157,184,199,214). */
const char* qc_last_error(void);

/* Introspection: which device formulation the handle selected
 * ("diagW-6x6-uniform", "diagW-6x6" or "dense-12x12"), and ABI version. */
const char* qc_kernel_name(const qc_handle* h);
int qc_abi_version(void);
/* ABI v5.  Guard for callers compiled separately from the library: pass QC_ABI_VERSION, sizeof(qc_params),
 * sizeof(qc_batch_in) and sizeof(qc_batch_out) as the CALLER's header defines them; anything but QC_OK (QC_ERR_ABI, with
 * the two sides spelled out in qc_last_error) means the structs this library reads are not the ones the caller fills
 * (qc_batch_in has grown with every revision and carries no size field) and no other entry point may be used.  The
 * C++ adapter's constructor and the Python loader call it (it needs no device); since ABI v6 the constructor performs the
 * same check itself (qc_create_abi), so this entry point is a convenience for an early, device-free diagnosis.
 * (The reference's constructor contract, balance_controller.hpp:85-88, has no analogue: it is header-only C++.) */
int qc_check_abi(int abi_version, size_t sizeof_params, size_t sizeof_batch_in, size_t sizeof_batch_out);
#define QC_CHECK_ABI() qc_check_abi(QC_ABI_VERSION, sizeof(qc_params), sizeof(qc_batch_in), sizeof(qc_batch_out))

/* ABI v4.  Which kernel instantiation a batch of n robots would run on (kin = joint_q given, warm = warm-start
 * words given): lanes per robot, kernel mode (1 one fill per wave, 2 one fill
 * and one wave per SIMD with register-resident constants; batches that leave SIMDs idle even so race 2 or 4 pivoting
 * strategies per robot there, `strategies`; 3 paired waves - two one-lane waves per workgroup, the last to arrive
 * finishes both waves' stragglers: 6x6 forms from 524 288 robots on), form (0 uniform 6x6, 1 general 6x6, 2 dense 12x12),
 * robots per wave, grid size, and the workgroups of that kernel the device holds at once (the occupancy query the
 * heuristics use). */
typedef struct qc_launch_info {
  int32_t lanes_per_robot;
  int32_t mode;
  int32_t form;
  int32_t strategies; /* four lanes per robot, one-fill kernels: pivoting strategies racing per robot (1, 2 or 4) */
  int64_t chunk;
  int64_t blocks;
  int64_t resident_workgroups;
  int64_t lds_bytes;
} qc_launch_info;
int qc_query_launch(qc_handle* h, size_t n, int kin, int warm, qc_launch_info* out);

/* ABI v4.  Development / test interface: explicit overrides of the launch heuristics and solver constants (the
 * library reads NO environment variables).  Keys: "group" (lanes per robot: 0 = heuristic, 1, 2, 4), "one_fill"
 * (-1 heuristic or 1: every launch runs one-fill workgroups; 0 fails with QC_ERR_INVALID), "chunk" (robots per wave,
 * 0 = heuristic; beyond one fill - 64 / lanes per robot - QC_ERR_INVALID at launch),
 * "wave_slots" (resident workgroups assumed, 0 = occupancy query),
 * "race" (-1 heuristic; 0 or 1: one strategy per robot; 2, 4: at most that many racing in the 4-lane one-fill kernels.  With the
 * race on - the default for cold batches - a wave forks its last running robots onto idle lanes with a second drop rule, so a robot's
 * `iterations` (and, under a small max_iter, QC_SOLVED vs QC_MAX_ITER) depend on which robots share its wave, i.e. on the batch
 * layout; the forces agree to the KKT tolerance either way.  0 is the deterministic mode: one walk per robot whatever its neighbours),
 * "pair" (-1 heuristic, 0 never, 1 whenever one lane per robot on a 6x6 form: the paired-waves kernel, mode 3), "pair_th"
 * (its hand-over threshold, <= 32), "pair_refill" (free lane groups that trigger a refill, 1 ... 16), "pair_solo" (0: pairs in the last round of workgroups too),
 * "force_general" / "force_dense" (run the more general formulation on weights that would allow the
 * specialised one; same minimiser), "auto_dense" (1, default: a handle whose max diag(S) / min diag(W) exceeds 3e8 - regularisation
 * weights 300 times further below S than the reference's - runs the dense 12x12 form although its W is diagonal, because the 6x6 dual
 * forms lose digits that matter there, eps (S/w) |b|; 0: it keeps the 6x6 form), "clamp_steps" (clamp steps a cold-started robot takes before its first ratio test in
 * the one-fill kernels; 0 = the kernel's rule: five on one or two lanes per robot, one on four),
 * "tol_d" (relative multiplier tolerance), "polish" (1, default: the first time a robot would be accepted while its
 * smallest multiplier lies inside the noise band +-tol_d |grad|, that face is released once instead; 0: accept at -tol_d |grad|
 * straight away, round 5's rule - up to tol_d |grad| / (2 w) from the minimiser for very small W), "max_iter" (<= 0: back to qc_params.max_iter), "probe_batch_load"
 * (1: skip the solver iterations - load, assemble, store only; every robot then reports QC_MAX_ITER; 0: back to the
 * handle's own cap).  "force_general" / "force_dense" / "max_iter" / "probe_batch_load" restore what qc_create was given,
 * whatever the order of the calls.
 * Calls that change device constants synchronise the device first.  Returns QC_ERR_INVALID for an unknown key. */
int qc_set_tuning(qc_handle* h, const char* key, double value);

/* Commander mode: the body of the reference's commander loop (commander_node.cpp:344-531) on the device.  Instead of a
 * host-supplied desired COM state (qc_batch_in.Rwb_d / x_d / xdot_d / w_d), each robot carries a qc_commander_state that
 * the tick itself advances, from the measured COM state and the user's body twist (cmd_vel, commander_node.cpp:191-202):
 *   1. a fresh command overwrites Vb and sets cmd_pending;
 *   2. standing latches once |x(2) - stand_height| < stand_tol (strict, math::almost_equal; never reset);
 *   3. standing and gait_running already set: a pending command is applied - (Rwb_d, x_d) = integrate_twist_yaw((Rwb, x),
 *      Vb, cmd_dt) (trajectory.cpp:29-69) with x_d(2) = stand_height, (xdot_d, w_d) = Ad_T(Rwb, x) Vb (rigid3d.cpp:259-271,
 *      i.e. Rwb^T (v - x x w) and Rwb^T w) - and the gait clock, the contact rule and the foothold planner run as in
 *      qc_control_batch; standing but not yet running: gait_running is set and nothing else happens this tick;
 *   4. until the gait runs, the gait map is make_stance_gait(): all legs stance, the phases do not move, no planning.
 * The QP and the stance J^T torques run every tick with the state's current desired values.  (stand_cmd_received is not
 * modelled: calling qc_tick_batch for a robot stands for it.)  INTEGRATION.md names the two reference quirks kept here. */
typedef struct qc_commander_state {
  int32_t standing;     /* the stand height was reached (latched)                                 */
  int32_t gait_running; /* the gait clock has been started                                        */
  int32_t cmd_pending;  /* cmd_vel_received: a command waits to be applied                        */
  int32_t reserved;
  double Vb[6];         /* latest body twist (vx, vy, vz, wx, wy, wz)                             */
  double Rwb_d[9];      /* desired state fed to the controller, row-major                         */
  double x_d[3];
  double xdot_d[3];
  double w_d[3];
} qc_commander_state;

/* Per-call arguments of qc_tick_batch (DEVICE pointers). */
typedef struct qc_command_in {
  size_t struct_size;           /* = sizeof(qc_command_in); checked (a struct that grows carries its size)   */
  const double* twist;          /* [n][6] commands; must be readable when `fresh` is given, used where fresh[i] != 0 */
  const uint8_t* fresh;         /* [n] 1 = a command arrived for this robot since its previous tick; NULL = none    */
  qc_commander_state* state;    /* [n] IN/OUT, initialise with qc_commander_state_init                     */
  double stand_height;          /* x_stand(2), 0.26 (commander_node.cpp:355)                               */
  double stand_tol;             /* 0.005 (commander_node.cpp:387)                                          */
  double cmd_dt;                /* user command integration step, 0.001 (commander_node.cpp:344); not the tick period */
} qc_command_in;

/* The reference's values: struct_size set, no arrays, stand_height 0.26, stand_tol 0.005, cmd_dt 0.001. */
void qc_default_command(qc_command_in* cmd);
/* Host helper: the commander's initial state for n robots (commander_node.cpp:346-367): flags 0, Vb 0, Rwb_d = I,
 * x_d = x_stand (NULL = (0, 0, 0.26)), xdot_d = w_d = 0. */
void qc_commander_state_init(qc_commander_state* states, size_t n, const double x_stand[3]);
/* The complete tick in commander mode: asynchronous on `stream`, no host synchronisation (graph-capturable).  `in` carries
 * the measured state and the tick's arrays like qc_control_batch with joint_q, joint_qdot, gait_phase, gait_dt and
 * swing_state given; its Rwb_d / x_d / xdot_d / w_d must be NULL (the desired state lives in cmd->state), stance,
 * swing_pos and swing_vel must be NULL, and out->joint_tau is required.  QC_ERR_INVALID otherwise, nothing launched. */
int qc_tick_batch(qc_handle* h, size_t n, const qc_batch_in* in, const qc_command_in* cmd, const uint32_t* warm,
                  const qc_batch_out* out, void* stream);

/* Closing the loop: one step of the plant the controller itself assumes, BalanceController::dynamics()
 * (balance_controller.cpp:237-272) - ONE rigid body with world-frame forces at the feet - so that a batch advances on the
 * device between two qc_control_batch launches.  Per robot (mass and Ib from the handle, g = 9.81):
 *   f_i = -Rwb grf_body_i,  r_i = foot_world_i - x,  a = (sum f_i) / m - (0, 0, g),
 *   wdot = Iw^-1 (sum r_i x f_i - w x (Iw w)),  Iw = Rwb Ib Rwb^T,
 *   xdot' = xdot + dt a,  x' = x + dt xdot',  w' = w + dt wdot,  Rwb' = Exp(dt w') Rwb   (semi-implicit Euler, Rodrigues).
 * `w` is the angular velocity in the WORLD frame, as control() takes it.  `grf_body` is what qc_control_batch wrote (negated,
 * body frame; 0 for swing legs and failed robots - a failed QP is free fall for that step).  There is NO contact model: the
 * forces are applied as given and a stance foot is where foot_world says it is; the body has no legs, so joints and the
 * leg-level tick (joint_q, qc_tick_batch) are outside this model.  Each robot's inputs are all read before any of its outputs
 * is written: the state is updated in place, and `feet` - Rwb'^T (foot_world_i - x'), the array the next qc_control_batch
 * reads - may be any array of that layout, foot_world included.  All pointers are DEVICE pointers. */
typedef struct qc_plant_io {
  size_t struct_size;        /* = sizeof(qc_plant_io); checked, like qc_command_in                         */
  double *Rwb, *x, *xdot, *w; /* [n][9], [n][3], [n][3], [n][3] IN/OUT                                       */
  const double* grf_body;    /* [n][4][3] qc_batch_out.grf_body                                            */
  const double* foot_world;  /* [n][4][3] world positions of the four feet                                 */
  double* feet;              /* [n][4][3] OUT, optional (NULL): body-frame feet of the new state           */
  double dt;                 /* seconds, finite, > 0                                                       */
} qc_plant_io;
/* struct_size set, pointers NULL, dt = 1/300 (mit_cheetah_config.yaml:3). */
void qc_default_plant(qc_plant_io* io);
/* Asynchronous on `stream`, no host synchronisation; n == 0 launches nothing.  QC_ERR_INVALID (message starting with
 * "qc_plant_step_batch:", nothing launched) for a null required pointer, a wrong struct_size, a dt that is not finite and
 * > 0, or a handle whose Ib is not finite, symmetric and positive definite (qc_create itself does not ask that of Ib). */
int qc_plant_step_batch(qc_handle* h, size_t n, const qc_plant_io* io, void* stream);

/* Closing the loop around the complete tick: one step of a LEGGED plant under the joint torques qc_control_batch (with joint_q /
 * joint_tau) or qc_tick_batch wrote - a single rigid body on massless legs.  Per robot (mass, Ib and the kinematic constants
 * from the handle, g = 9.81):
 *   contact mask: `stance` bytes if given; else the phase rule of qc_batch_in.gait_phase (1e-12 slack, `gait_duty` or the
 *     handle's value) on the phases AS THE TICK LEFT THEM (the plant never advances the clock); else all stance.  `cmd_state`,
 *     if given, overrides all of it for a robot whose gait_running is 0: all stance.
 *   stance leg i: p_i = FK(q_i), J_i = legJacobian(q_i); the force the torque encodes, g_i = J_i^-T tau_i (closed form while
 *     max(eps, 64 eps (sum |l|)^3) <= |det J_i| <= 2^52, the pseudo-inverse of J_i^T and bit i of `flags` otherwise), is in
 *     grf_body's convention, so f_i = -Rwb g_i acts on the body at r_i = Rwb p_i, and the foot is pinned at c_i = x + r_i.
 *   swing leg: no force on the body; its joints are three double integrators with the reflected inertia leg_inertia:
 *     qdot' = qdot + dt tau / I,  q' = q + dt qdot'.
 *   body: exactly qc_plant_step_batch's step from sum f_i and sum r_i x f_i.
 *   stance leg afterwards: p_i' = Rwb'^T (c_i - x'), q_i' = legInverseKinematics(p_i') (kinematics.cpp:117-160 with its d > 1
 *     clamp), qdot_i' = wrapPI(q_i' - q_i) / dt; a clamped leg (foot out of reach) or a NaN leg (d < -1) sets bit 4 + i of
 *     `flags`, and the NaN propagates as in the reference.
 * There is no ground (a leg entering stance is pinned wherever its foot is), no leg mass, no gravity on the joints; the
 * torque clamp of the tick is the plant's actuator limit.  INTEGRATION.md, "Closing the loop around the tick", has the limits.
 * Every input of a robot is read before any output of that robot is written: Rwb, x, xdot, w, joint_q and joint_qdot are
 * updated in place.  All pointers are DEVICE pointers. */
typedef struct qc_leg_plant_io {
  size_t struct_size;           /* = sizeof(qc_leg_plant_io); checked                                              */
  double *Rwb, *x, *xdot, *w;   /* [n][9], [n][3], [n][3], [n][3] IN/OUT                                           */
  double *joint_q, *joint_qdot; /* [n][4][3] IN/OUT                                                                */
  const double* joint_tau;      /* [n][4][3] qc_batch_out.joint_tau                                                */
  const uint8_t* stance;        /* [n][4] optional                                                                 */
  const double* gait_phase;     /* [n][4] optional, as the tick left it                                            */
  const double* gait_duty;      /* [n] optional (NULL: the handle's stance_phase)                                  */
  const qc_commander_state* cmd_state; /* [n] optional: gait_running == 0 -> all stance                            */
  double* foot_world;           /* [n][4][3] OUT, optional: x + Rwb FK(q) of the state the step read - the pinned
                                   contact point c_i of a stance leg                                               */
  int32_t* flags;               /* [n] OUT, optional: bit l singular Jacobian, bit 4 + l out of reach (stance leg l) */
  double leg_inertia[3];        /* kg m^2 (hip, thigh, calf), finite and > 0: the reference has no number for it   */
  double dt;                    /* seconds, finite, > 0                                                            */
} qc_leg_plant_io;
/* struct_size set, pointers NULL, dt = 1/300, leg_inertia = 0 (the caller must give one). */
void qc_default_leg_plant(qc_leg_plant_io* io);
/* Asynchronous on `stream`, no host synchronisation (graph-capturable); n == 0 launches nothing and returns QC_OK.
 * QC_ERR_INVALID (message starting with "qc_leg_plant_step_batch:", nothing launched) for a null required pointer (the
 * handle, io, Rwb, x, xdot, w, joint_q, joint_qdot, joint_tau), a wrong struct_size, a dt or a leg_inertia entry that is not
 * finite and > 0, or a handle whose mass or Ib qc_plant_step_batch refuses. */
int qc_leg_plant_step_batch(qc_handle* h, size_t n, const qc_leg_plant_io* io, void* stream);

/* Certifying a batch: the solver-independent KKT certificate of the forces qc_control_batch returned, and their Lagrange
 * multipliers, on the device.  Per robot, from the SAME qc_batch_in the solve read (r_i = Rwb p_i with p_i from `feet`, or from
 * joint_q by the forward kinematics; b from the PD law) and the handle's mu, fzmin, fzmax and FULL S (6x6) and W (12x12),
 * whatever formulation the solver ran:
 *   f_i = -Rwb grf_body_i,   grad = 2 (A^T S (A f - b) + W f)                               (world frame)
 *   contact mask: `stance` bytes if given; else the phase rule on gait_phase AS IT IS NOW (gait_duty or the handle's value);
 *     else all stance.  gait_dt, swing_pos, swing_vel, joint_qdot and swing_state are ignored: the certificate never advances
 *     a clock and never writes to `in`.
 *   primal [N]: the largest of |fx| - mu fz, |fy| - mu fz, fzmin - fz, fz - fzmax over the stance feet (a swing foot counts 0).
 *   active rows per stance foot and axis, a code 0 none, 1 lower row, 2 upper row, 3 both: x lower is fx = -mu fz, x upper
 *     fx = +mu fz, a row being active when its slack is <= act_tol (1 + mu |fz|); y alike; z lower is fz = fzmin (slack <=
 *     act_tol (1 + fzmin)), z upper fz = fzmax (slack <= act_tol (1 + fzmax)).
 *   multipliers with one row active (s = -1 lower, +1 upper): lam_x = -s_x g_x, lam_y = -s_y g_y,
 *     lam_z = s_z (mu (lam_x + lam_y) - g_z); an axis without a row has lam = 0 and contributes |g| to the residual
 *     (z: |mu (lam_x + lam_y) - g_z|), an axis with one row max(0, -lam).
 *   BOTH rows of an axis active (the apex of the pyramid at fz = 0 = fzmin, or fzmin = fzmax): x, y: lam = |g|, carried by the
 *     row on the side -sign(g) - the pair of least sum, the choice that can satisfy the z row - and the axis contributes 0;
 *     z: the equality leaves lam_z free, the axis contributes 0 and lam_z reports the net value mu (lam_x + lam_y) - g_z
 *     (upper minus lower).
 *   stationarity: the largest contribution over the stance feet / (1 + |grad|_2).
 * Non-finite inputs propagate as NaN; nothing is clamped.  Commander mode (qc_tick_batch) is out of scope: its desired state
 * lives in qc_commander_state, not in qc_batch_in. */
typedef struct qc_certify_summary {
  int64_t n_fail;            /* robots with !(primal <= primal_tol) || !(stationarity <= stat_tol) or the swing flag (a NaN fails) */
  int64_t n_nonfinite;       /* robots whose primal or stationarity residual is not finite                                     */
  int64_t n_swing_nonzero;   /* robots with a non-zero force on a swing foot                                                   */
  double worst_primal;       /* the largest FINITE primal residual (NaN if none is finite)                                     */
  double worst_stationarity; /* the largest FINITE stationarity residual (NaN if none is finite)                               */
  int64_t arg_primal;        /* its robot, the lowest index on a tie; -1 if none is finite                                     */
  int64_t arg_stationarity;
} qc_certify_summary;

/* Per-call arguments of qc_certify_batch (DEVICE pointers).  Every output is optional; at least one must be given. */
typedef struct qc_certify_io {
  size_t struct_size;        /* = sizeof(qc_certify_io); checked                                                     */
  const double* grf_body;    /* [n][4][3] qc_batch_out.grf_body                                                      */
  double act_tol;            /* active-row tolerance, finite and >= 0                                                */
  double primal_tol;         /* bars of qc_certify_summary.n_fail, finite and >= 0                                   */
  double stat_tol;
  double* primal;            /* [n]                                                                                  */
  double* stationarity;      /* [n]                                                                                  */
  double* lambda;            /* [n][4][3] (x, y, z) multipliers as defined above: raw values, negative where the point
                                is not optimal; 0 on an axis without an active row and for swing feet               */
  double* grad;              /* [n][12] world frame                                                                  */
  uint8_t* active;           /* [n][4]: x code | y code << 2 | z code << 4; 0x80 for a swing foot                    */
  int32_t* flags;            /* [n]: bit 0 a swing foot carries force, bit 1 a residual is not finite                */
  qc_certify_summary* summary; /* one struct, written by a second, one-workgroup kernel                              */
} qc_certify_io;
/* struct_size set, pointers NULL, act_tol = 1e-7, primal_tol = 1e-7, stat_tol = 1e-8. */
void qc_default_certify(qc_certify_io* io);
/* Asynchronous on `stream`, no host synchronisation (graph-capturable); n == 0 launches nothing and returns QC_OK.  The
 * summary goes through a partial buffer the handle owns, reduced without atomics: it is deterministic and bit-equal to
 * reducing the per-robot arrays, works with all of them NULL, and two calls with a summary on one handle must be ordered on
 * the device (one stream, or an event between them).  QC_ERR_INVALID (message starting with "qc_certify_batch:", nothing
 * launched) for a null handle, `in` or `io`, a wrong struct_size, a tolerance that is not finite and >= 0, no output
 * requested at all, a missing grf_body, a missing state array (Rwb, Rwb_d, x, xdot, w, x_d, xdot_d, w_d), neither feet nor
 * joint_q, or n beyond one launch. */
int qc_certify_batch(qc_handle* h, size_t n, const qc_batch_in* in, const qc_certify_io* io, void* stream);

/* Sensitivity of a solved batch: the adjoint of the balance QP on the active face of the forces qc_control_batch returned.  Per
 * robot the solve minimises (A f - b)^T S (A f - b) + f^T W f over the world-frame forces f (12 values) under the pyramid rows
 * described at qc_certify_batch; A = [I I I I; [r_1]x ... [r_4]x], r_i = Rwb p_i (p_i from `feet`, or from joint_q by the forward
 * kinematics), b from the PD law, the handle's FULL S (6x6) and W (12x12) whatever formulation the solver ran; H = 2 (A^T S A + W).
 * Inputs are the SAME qc_batch_in the solve read (contact mask resolved as qc_certify_batch resolves it; gait_dt and the swing
 * arrays are ignored, `in` is never written), the forces and a cotangent grf_bar on them.
 *   The face: each stance foot's axes get qc_certify_batch's codes at act_tol (0 none, 1 lower, 2 upper, 3 both), and f = Z y + f0:
 *     z code != 0: fz is pinned; z code 0: fz is free.  x (or y) code 0: free; code 1 or 2: fx = -mu fz or +mu fz - tied to fz if fz
 *     is free, pinned otherwise.  A code 3 on any axis of a foot pins the whole foot and sets bit 0 of `flags`: the derivative is
 *     one-sided there.  Swing feet are pinned.  A failed robot has all-zero forces, so every stance foot of it is pinned and
 *     flagged and its adjoint is 0.
 *   f_bar = -Rwb grf_bar (Rwb held fixed);  adjoint z = Z (Z^T H Z)^-1 Z^T f_bar (world frame, 0 in pinned coordinates);
 *   b_bar = 2 S A z;  r_bar_i = -2 (z_i x v_ang + f_i x q_ang) with v = S (A f - b), q = S A z;  feet_bar_i = Rwb^T r_bar_i, the
 *   cotangent of the body-frame foot position whether it came from `feet` or from the kinematics of joint_q;
 *   x_bar, xdot_bar, w_bar, x_d_bar, xdot_d_bar, w_d_bar: b_bar pulled back through the PD law at fixed Rwb and Rwb_d, exactly
 *   as the library evaluates that law (the kff terms on xdot_d[0], xdot_d[1] and w_d included).
 * NOT produced: the cotangents of Rwb and Rwb_d - qc_sensitivity_rot_batch below makes them from b_bar and feet_bar; weak activity -
 * a row whose multiplier is about 0 counts as active like any other (qc_certify_batch's lambda shows such rows).  The cotangents of the
 * handle's own parameters - mu, fzmin, fzmax, the weights, the gains, mass and Ib - come from qc_sensitivity_param_batch below, given
 * this call's adjoint.  Commander mode: the desired state is qc_commander_step_batch's, given here as Rwb_d / x_d / xdot_d / w_d; x_d_bar,
 * xdot_d_bar and w_d_bar go on to qc_commander_step_adjoint_batch.
 * The reduced system is solved as a fixed 12x12 LDL^T; a pivot that is not positive and finite sets bit 1 of `flags` and makes
 * every output of that robot NaN.  Non-finite inputs propagate as NaN; nothing is clamped. */
typedef struct qc_sensitivity_io {
  size_t struct_size;        /* = sizeof(qc_sensitivity_io); checked                                                 */
  const double* grf_body;    /* [n][4][3] qc_batch_out.grf_body                                                      */
  const double* grf_bar;     /* [n][4][3] cotangent on grf_body                                                      */
  double act_tol;            /* active-row tolerance, finite and >= 0                                                */
  double* adjoint;           /* [n][12] z, world frame                                                               */
  double* b_bar;             /* [n][6]                                                                               */
  double* feet_bar;          /* [n][4][3] body frame                                                                 */
  double *x_bar, *xdot_bar, *w_bar, *x_d_bar, *xdot_d_bar, *w_d_bar; /* [n][3] each                                   */
  int32_t* flags;            /* [n]: bit 0 a foot sits on both rows of an axis (one-sided), bit 1 a bad pivot        */
} qc_sensitivity_io;
/* struct_size set, pointers NULL, act_tol = 1e-7. */
void qc_default_sensitivity(qc_sensitivity_io* io);
/* Asynchronous on `stream`, no host synchronisation (graph-capturable); n == 0 launches nothing and returns QC_OK.  Every output
 * is optional; at least one must be given.  QC_ERR_INVALID (message starting with "qc_sensitivity_batch:", nothing launched) for a
 * null handle, `in` or `io`, a wrong struct_size, an act_tol that is not finite and >= 0, a missing grf_body or grf_bar, no output
 * requested at all, a missing state array (Rwb, Rwb_d, x, xdot, w, x_d, xdot_d, w_d), neither feet nor joint_q, or n beyond one
 * launch. */
int qc_sensitivity_batch(qc_handle* h, size_t n, const qc_batch_in* in, const qc_sensitivity_io* io, void* stream);

/* The rotation cotangents of a solved batch: what qc_sensitivity_batch leaves out.  Given the SAME qc_batch_in, the forces, the
 * cotangent grf_bar on them and the b_bar and feet_bar qc_sensitivity_batch wrote for that grf_bar (the adjoint itself is not needed;
 * no solve is repeated), with R = Rwb, Rd = Rwb_d, f_i = -R grf_body_i, ba = b_bar[3:6], p_i the body-frame foot (`feet`, or joint_q
 * through the forward kinematics), the ENTRYWISE cotangents (row-major, dL / dR_ab of the expressions exactly as the library
 * evaluates them, the nine entries taken as independent) are the sum of
 *   the output transform grf_body_i = -R^T f_i at fixed f:   R_bar += -sum_i f_i grf_bar_i^T
 *   the lever arms r_i = R p_i:                              R_bar += sum_i (R feet_bar_i) p_i^T
 *   Iw = R Ib R^T in b_ang = Iw al + w_d x (Iw w_d):         Iw_bar = ba al^T + (ba x w_d) w_d^T,  R_bar += Iw_bar R Ib^T + Iw_bar^T R Ib
 *   the rotation error e = log(Rd R^T) in al = kp_w e + ...: e_bar = kp_w o (Iw^T ba), Re_bar its pull-back through the library's
 *     Eigen-convention log on the branch it took,            R_bar += Re_bar^T Rd,   Rd_bar = Re_bar R.
 * Rwb_rot_bar and Rwb_d_rot_bar are the world-frame left-tangent projections: for R <- exp([delta]x) R the cotangent of delta is
 * axial(R_bar R^T), axial(M) = (M32 - M23, M13 - M31, M21 - M12); the same form for Rd.  These are what a caller that keeps its
 * rotations on the manifold wants; the entrywise ones are what an autodiff that holds nine numbers wants.
 * Where the error is exactly the identity the log's smooth limit is differentiated, not the select that returns 0 there.  At an
 * error angle of exactly pi the log is discontinuous for any implementation: the derivative is that of the branch evaluated.
 * As every output of qc_sensitivity_batch this is the gradient ON THE ACTIVE FACE: valid while the working set holds, one-sided for
 * robots with bit 0 of its flags, NaN for robots with bit 1 (their b_bar and feet_bar are NaN and every output here with them).
 * Non-finite inputs propagate as NaN; nothing is clamped.  Rwb_d must be in `in`: in commander mode it is
 * qc_commander_step_batch's, and Rwb_d_bar goes on to qc_commander_step_adjoint_batch. */
typedef struct qc_sensitivity_rot_io {
  size_t struct_size;        /* = sizeof(qc_sensitivity_rot_io); checked                                             */
  const double* grf_body;    /* [n][4][3] qc_batch_out.grf_body                                                      */
  const double* grf_bar;     /* [n][4][3] cotangent on grf_body                                                      */
  const double* b_bar;       /* [n][6]    qc_sensitivity_io.b_bar for that grf_bar                                   */
  const double* feet_bar;    /* [n][4][3] qc_sensitivity_io.feet_bar for that grf_bar                                */
  double* Rwb_bar;           /* [n][9] entrywise, row-major                                                          */
  double* Rwb_d_bar;         /* [n][9]                                                                               */
  double* Rwb_rot_bar;       /* [n][3] world-frame left tangent                                                      */
  double* Rwb_d_rot_bar;     /* [n][3]                                                                               */
} qc_sensitivity_rot_io;
/* struct_size set, pointers NULL. */
void qc_default_sensitivity_rot(qc_sensitivity_rot_io* io);
/* Asynchronous on `stream`, no host synchronisation (graph-capturable; ordered behind qc_sensitivity_batch on the same stream it
 * needs no event); n == 0 launches nothing and returns QC_OK.  Every output is optional; at least one must be given.
 * QC_ERR_INVALID (message starting with "qc_sensitivity_rot_batch:", nothing launched) for a null handle, `in` or `io`, a wrong
 * struct_size, no output requested at all, a missing grf_body, grf_bar, b_bar or feet_bar, a missing state array (Rwb, Rwb_d, x,
 * xdot, w, x_d, xdot_d, w_d - commander mode keeps the desired ones in its own record and is refused by this), neither feet nor
 * joint_q, or n beyond one launch. */
int qc_sensitivity_rot_batch(qc_handle* h, size_t n, const qc_batch_in* in, const qc_sensitivity_rot_io* io, void* stream);

/* The parameter cotangents of a solved batch: the gradient of <grf_bar, grf_body> in the handle's own qc_params - the gains kp_p, kd_p,
 * kp_w, kd_w and kff, the weights S and W, mu, fzmin, fzmax and the controller's mass and Ib.  Given the SAME qc_batch_in, the forces,
 * the cotangent grf_bar on them and the `adjoint` z qc_sensitivity_batch wrote for that grf_bar (no solve is repeated).
 * A parameter cotangent is QC_PARAM_COUNT = 211 doubles in the order of the double members of qc_params: mu, mass, fzmin, fzmax, Ib[9],
 * S[36], W[144], kff[6], kp_p[3], kd_p[3], kp_w[3], kd_w[3].  Matrices are ENTRYWISE and row-major, the entries taken as independent
 * (Rwb_bar's convention).  S_bar and W_bar are therefore the UNSYMMETRISED forms below: qc_create accepts symmetric S and W only, so
 * only <S_bar, dS> with a symmetric dS (and W alike) is a derivative of anything; symmetrise them if a single entry is to be read.
 * On the active face at fixed codes, with f the world forces, f_bar = -Rwb grf_bar, u = A f - b, v = S u, g = 2 (A^T v + W f),
 * b_bar = 2 S A z, rho = f_bar - 2 (A^T S A z + W z):
 *   S_bar = -2 (A z) u^T,   W_bar = -2 z f^T;
 *   mass, kff, kp_p, kd_p, kp_w, kd_w: b_bar pulled back through the PD law line by line, exactly as the library evaluates it (mass
 *     enters three times - m a, kff[2] m 9.81 inside a[2], and -9.81 m -, kff[5] acts on the SECOND angular component);
 *   Ib_bar = Rwb^T (ba al^T + (ba x w_d) w_d^T) Rwb with ba = b_bar[3:6] (qc_sensitivity_rot_batch's Iw_bar);
 *   mu_bar: over the stance feet, with sx, sy in {-1, 0, +1} from the x / y codes 1 / 2 / 0,
 *     <rho_l, (sx f_lz, sy f_lz, 0)> - [fz free] z_lz (sx g_lx + sy g_ly);
 *   fzmin_bar: over the feet with z code 1, <rho_l, (sx mu, sy mu, 1)>;  fzmax_bar: the same over the feet with z code 2.
 * mass_bar and Ib_bar are the gradient of the CONTROLLER's use of mass and Ib (the wrench target); what a plant makes of the same two
 * numbers is another function (qc_plant_step_adjoint_batch produces no such cotangent).  A foot with a code 3 on any axis adds nothing
 * to mu_bar, fzmin_bar and fzmax_bar (bit 0 of qc_sensitivity_batch's flags marks that robot: one-sided).  A failed robot (all forces
 * zero) gives a zero row, a NaN adjoint (flags bit 1) a NaN row - and a NaN sum.  Non-finite inputs propagate; nothing is clamped.
 * Commander mode is out of scope. */
typedef struct qc_sensitivity_param_io {
  size_t struct_size;        /* = sizeof(qc_sensitivity_param_io); checked                                           */
  const double* grf_body;    /* [n][4][3] qc_batch_out.grf_body                                                      */
  const double* grf_bar;     /* [n][4][3] cotangent on grf_body                                                      */
  const double* adjoint;     /* [n][12]   qc_sensitivity_io.adjoint for that grf_bar, at the same act_tol            */
  double act_tol;            /* active-row tolerance, finite and >= 0: the one qc_sensitivity_batch was given        */
  double* param_bar_rows;    /* [n][QC_PARAM_COUNT] per robot                                                        */
  double* param_bar;         /* [QC_PARAM_COUNT] the sum over the batch, written by a second, one-workgroup kernel   */
} qc_sensitivity_param_io;
/* struct_size set, pointers NULL, act_tol = 1e-7. */
void qc_default_sensitivity_param(qc_sensitivity_param_io* io);
/* Asynchronous on `stream`, no host synchronisation (graph-capturable; ordered behind qc_sensitivity_batch on the same stream it
 * needs no event); n == 0 launches nothing and returns QC_OK (param_bar is then left as it is).  Both outputs are optional; at least
 * one must be given.  The sum goes through a partial buffer the handle owns, reduced without atomics in an order that depends on n
 * alone: it is bit-reproducible, the same with and without param_bar_rows, and independent of what an earlier call left in the
 * buffer; two calls with a param_bar on one handle must be ordered on the device (one stream, or an event between them).
 * QC_ERR_INVALID (message starting with "qc_sensitivity_param_batch:", nothing launched) for a null handle, `in` or `io`, a wrong
 * struct_size, an act_tol that is not finite and >= 0, no output requested at all, a missing grf_body, grf_bar or adjoint, a missing
 * state array (Rwb, Rwb_d, x, xdot, w, x_d, xdot_d, w_d), neither feet nor joint_q, or n beyond one launch. */
int qc_sensitivity_param_batch(qc_handle* h, size_t n, const qc_batch_in* in, const qc_sensitivity_param_io* io, void* stream);

/* The joint-angle cotangents of a fused tick (joint_q -> forward kinematics -> QP -> clamped J^T -> joint_tau): the two ends
 * qc_sensitivity_batch leaves open, in one kernel.  Per robot and leg l, with q = joint_q_l, p the forward kinematics of q,
 * J[r][c] = d p_r / d q_c its exact Jacobian (the matrix of the torque map), H_r = d^2 p_r / d q^2 and g = grf_body_l: the tick's
 * torque is tau_raw = J^T g clamped by two compares to [tau_min, tau_max] of qc_set_kinematics, emitted for a stance leg of a robot
 * with status 0 and 0 otherwise.  Given the optional cotangents joint_tau_bar, feet_bar, grf_bar_in and joint_q_bar_in (a missing
 * one counts as zero):
 *   the mask    m_c = 1 where !(tau_raw_c < tau_min) && !(tau_raw_c > tau_max) - equality passes, a NaN passes and propagates -,
 *               m = 0 for a swing leg and for a robot with status != 0;  s = m o joint_tau_bar_l
 *   grf_bar_l     = grf_bar_in_l + J s                       body frame: the cotangent on grf_body that qc_sensitivity_batch takes
 *   joint_q_bar_l = joint_q_bar_in_l + (sum_r g_r H_r) s + J^T feet_bar_l
 * The term J^T feet_bar_l is UNMASKED: a swing leg's feet_bar from qc_sensitivity_batch is zero already, and a caller's own loss on a
 * foot position must pass.  The two typical calls: the torque half alone in front of qc_sensitivity_batch (joint_tau_bar, and the
 * loss's direct cotangent on grf_body as grf_bar_in: grf_bar is the total that call takes), then the kinematics half behind it
 * (its feet_bar, and the first call's joint_q_bar as joint_q_bar_in, in place).
 * Of `in` the call reads joint_q and the contact mask, resolved as qc_certify_batch resolves it (`stance` bytes, else the phase rule
 * on gait_phase as it is now, else all stance); none of the state arrays is read or required, `in` is never written.
 * OUT OF SCOPE: the swing legs' PD torques - with swing references the joint_tau_bar of a swing leg is ignored -, commander mode, and
 * the cotangents of the kinematic constants and of tau_min / tau_max.  Non-finite inputs propagate; nothing is clamped.
 * Each output may be the SAME array as its `_in`: every input of a leg is read before any output of it is written, and a leg touches
 * its own rows only.  All pointers are DEVICE pointers. */
typedef struct qc_sensitivity_kin_io {
  size_t struct_size;           /* = sizeof(qc_sensitivity_kin_io); checked                                          */
  const double* grf_body;       /* [n][4][3] qc_batch_out.grf_body; required with joint_tau_bar                      */
  const int32_t* status;        /* [n]       qc_batch_out.status;   required with joint_tau_bar                      */
  const double* joint_tau_bar;  /* [n][4][3] cotangent on qc_batch_out.joint_tau; optional                           */
  const double* feet_bar;       /* [n][4][3] cotangent on the body-frame feet (qc_sensitivity_io.feet_bar); optional */
  const double* grf_bar_in;     /* [n][4][3] added to grf_bar; optional                                              */
  const double* joint_q_bar_in; /* [n][4][3] added to joint_q_bar; optional                                          */
  double* grf_bar;              /* [n][4][3] OUT, optional; needs joint_tau_bar                                      */
  double* joint_q_bar;          /* [n][4][3] OUT, optional                                                           */
} qc_sensitivity_kin_io;
/* struct_size set, pointers NULL. */
void qc_default_sensitivity_kin(qc_sensitivity_kin_io* io);
/* Asynchronous on `stream`, no host synchronisation (graph-capturable); n == 0 launches nothing and returns QC_OK.  No buffer is
 * kept on the handle.  QC_ERR_INVALID (message starting with "qc_sensitivity_kin_batch:", nothing launched) for a null handle, `in`
 * or `io`, a wrong struct_size, no output requested, none of joint_tau_bar, feet_bar and joint_q_bar_in given, joint_tau_bar
 * without grf_body or without status, grf_bar requested without joint_tau_bar, a missing joint_q, or n beyond one launch. */
int qc_sensitivity_kin_batch(qc_handle* h, size_t n, const qc_batch_in* in, const qc_sensitivity_kin_io* io, void* stream);

/* Differentiating a rollout: the reverse pass of qc_plant_step_batch.  Given the state BEFORE a step (Rwb, x, xdot, w), the grf_body
 * and foot_world that step read, its dt, and cotangents on what it wrote (Rwb', x', xdot', w' and the optional feet'), this writes
 * the cotangents of Rwb, x, xdot, w, grf_body and foot_world: the transpose-Jacobian of the step exactly as the library evaluates it.
 * Nothing is saved by the forward call; the step is recomputed.  Matrix cotangents are ENTRYWISE and row-major (dL / dR_ab, the nine
 * entries of Rwb taken as independent - qc_sensitivity_rot_io.Rwb_bar's convention, so the two add up); no left-tangent form is made.
 * With Rn = Rwb' = E Rwb, E = Exp(phi) = I + A K + B K^2, K = hat(phi), phi = dt w', the reverse pass is
 *   feet'_l = Rn^T d_l, d_l = foot_world_l - x':  Rn_bar += d_l feet_bar_l^T,  d_bar_l = Rn feet_bar_l,  foot_world_bar_l += d_bar_l,
 *                                                 x'_bar -= d_bar_l
 *   Rn = E Rwb:                                   E_bar = Rn_bar Rwb^T,  Rwb_bar += E^T Rn_bar
 *   E = Exp(phi):                                 phi_bar = vee(K_bar - K_bar^T) + (A_bar A1 + B_bar B1) phi,
 *                                                 K_bar = A E_bar + B (E_bar K^T + K^T E_bar),  A_bar = <E_bar, K>,  B_bar = <E_bar, K^2>,
 *                                                 A1 = (cos theta - A) / theta^2,  B1 = (A - 2 B) / theta^2 - evaluated as series in
 *                                                 theta^2 below theta = 1 (limits -1/3 and -1/12: at theta = 0 exactly the smooth limit
 *                                                 is differentiated, not the step's select) and as the quotients above it
 *   the semi-implicit Euler step, wdot = Rwb Ib^-1 Rwb^T (tau - w x (Rwb Ib Rwb^T w)) into Rwb_bar, w_bar and tau_bar, and
 *   tau = sum r_l x f_l, r_l = foot_world_l - x, f_l = -Rwb grf_body_l:  f_bar_l = fs_bar + tau_bar x r_l,  r_bar_l = f_l x tau_bar,
 *                                                 grf_bar_l = -Rwb^T f_bar_l,  Rwb_bar += -f_bar_l grf_body_l^T.
 * NOT produced: the cotangents of mass, Ib and dt (of mass and Ib, and of an external wrench: qc_plant_step_model_adjoint_batch,
 * include/qc_plant_model.h).  Outputs are written, not accumulated.  Non-finite inputs propagate as NaN;
 * nothing is clamped.  Each robot's inputs are all read before any of its outputs is written, and a robot touches its own rows
 * only: an output may be the SAME array as an input cotangent of the same layout (x_bar over x_next_bar, Rwb_bar over
 * Rwb_next_bar, foot_world_bar or grf_bar over feet_next_bar, ...), so backpropagation through time runs in place.  The six state
 * and force inputs are never written.  All pointers are DEVICE pointers. */
typedef struct qc_plant_adjoint_io {
  size_t struct_size;            /* = sizeof(qc_plant_adjoint_io); checked                                              */
  const double *Rwb, *x, *xdot, *w; /* [n][9], [n][3], [n][3], [n][3]: the state BEFORE the step                        */
  const double* grf_body;        /* [n][4][3] the forces the step read                                                  */
  const double* foot_world;      /* [n][4][3] the feet the step read                                                    */
  const double* Rwb_next_bar;    /* [n][9]    cotangents on the step's outputs: each optional (NULL = zero),            */
  const double* x_next_bar;      /* [n][3]    at least one given                                                        */
  const double* xdot_next_bar;   /* [n][3]                                                                              */
  const double* w_next_bar;      /* [n][3]                                                                              */
  const double* feet_next_bar;   /* [n][4][3] on qc_plant_io.feet                                                       */
  double* Rwb_bar;               /* [n][9]    outputs: each optional, at least one given                                */
  double *x_bar, *xdot_bar, *w_bar; /* [n][3] each                                                                      */
  double* grf_bar;               /* [n][4][3] on grf_body: the grf_bar qc_sensitivity_batch takes                       */
  double* foot_world_bar;        /* [n][4][3]                                                                           */
  double dt;                     /* seconds, finite, > 0: the step's                                                    */
} qc_plant_adjoint_io;
/* struct_size set, pointers NULL, dt = 1/300. */
void qc_default_plant_adjoint(qc_plant_adjoint_io* io);
/* Asynchronous on `stream`, no host synchronisation (graph-capturable); n == 0 launches nothing and returns QC_OK.
 * QC_ERR_INVALID (message starting with "qc_plant_step_adjoint_batch:", nothing launched) for a null handle or `io`, a wrong
 * struct_size, a dt that is not finite and > 0, no input cotangent at all, no output at all, a missing Rwb, x, xdot, w, grf_body or
 * foot_world, n beyond one launch, or a handle whose mass or Ib qc_plant_step_batch refuses. */
int qc_plant_step_adjoint_batch(qc_handle* h, size_t n, const qc_plant_adjoint_io* io, void* stream);

/* Differentiating the closed loop around the tick: the reverse pass of qc_leg_plant_step_batch.  Given the state BEFORE a step (Rwb,
 * x, xdot, w, joint_q, joint_qdot), the joint_tau and the contact inputs (stance / gait_phase / gait_duty / cmd_state, resolved as
 * that call resolves them) the step read, its dt and leg_inertia, and cotangents on what it wrote, this writes the cotangents of Rwb,
 * x, xdot, w, joint_q, joint_qdot and joint_tau: the transpose-Jacobian of the step exactly as the library evaluates it.  Nothing is
 * saved by the forward call; the step is recomputed.  Rwb's cotangents are ENTRYWISE (qc_plant_adjoint_io's convention).  Per leg,
 * with q', qd' the step's joint outputs and qn = q' of a stance leg:
 *   stance leg:  qn_bar = q'_bar + qd'_bar / dt,  q_bar = -qd'_bar / dt  (wrapPI has slope 1);  the inverse kinematics inverts the
 *                forward kinematics inside reach, so p'_bar = J(qn)^-T qn_bar;  p' = Rn^T (c - x'):  Rn_bar += (c - x') p'_bar^T,
 *                c_bar = Rn p'_bar,  x'_bar -= c_bar;  then qc_plant_step_adjoint_batch's body block to Rwb_bar, x_bar, xdot_bar,
 *                w_bar and the cotangents fs_bar, tau_bar of the net force and moment;  f = -Rwb g at r = Rwb FK(q), c = x + r:
 *                f_bar = fs_bar + tau_bar x r,  r_bar = f x tau_bar + c_bar,  x_bar += c_bar,  g_bar = -Rwb^T f_bar,
 *                Rwb_bar += r_bar FK(q)^T - f_bar g^T,  q_bar += J(q)^T Rwb^T r_bar;  g = J^-T tau:  joint_tau_bar = J^-1 g_bar,
 *                q_bar -= (sum_r g_r d^2 FK_r / dq^2) joint_tau_bar;  joint_qdot_bar = 0 (the step does not read it)
 *   swing leg:   s = qd'_bar + dt q'_bar;  q_bar = q'_bar,  joint_qdot_bar = s,  joint_tau_bar = dt s / leg_inertia.
 * UNDEFINED GRADIENTS: `flags` bit l - J(q_l) of stance leg l is outside the closed-form band (the step took the pseudo-inverse);
 * bit 4 + l - the step's inverse kinematics reported leg l out of reach, or J(qn_l) is outside the band.  A robot with any bit set
 * gets NaN in every output row.  Other non-finite inputs propagate; nothing is clamped.
 * NOT produced: a cotangent through the optional foot_world output, the cotangents of mass, Ib, leg_inertia, dt and the kinematic
 * constants; the contact mask is held (no gradient in the phases).  Outputs are written, not accumulated.  Each robot's inputs are
 * all read before any of its outputs is written, and a robot touches its own rows only: an output may be the SAME array as an input
 * cotangent of the same layout (joint_q_bar over joint_q_next_bar, x_bar over x_next_bar, ...).  The inputs are never written.
 * All pointers are DEVICE pointers. */
typedef struct qc_leg_plant_adjoint_io {
  size_t struct_size;               /* = sizeof(qc_leg_plant_adjoint_io); checked                                        */
  const double *Rwb, *x, *xdot, *w; /* [n][9], [n][3], [n][3], [n][3]: the state BEFORE the step                         */
  const double *joint_q, *joint_qdot; /* [n][4][3] before the step (joint_qdot's values are not read: the step is linear
                                       in a swing leg's and ignores a stance leg's)                                      */
  const double* joint_tau;          /* [n][4][3] the torques the step read                                               */
  const uint8_t* stance;            /* [n][4] optional: the contact inputs of the forward call                           */
  const double* gait_phase;         /* [n][4] optional                                                                   */
  const double* gait_duty;          /* [n] optional                                                                      */
  const qc_commander_state* cmd_state; /* [n] optional                                                                   */
  const double* Rwb_next_bar;       /* [n][9]    cotangents on the step's outputs: each optional (NULL = zero),          */
  const double* x_next_bar;         /* [n][3]    at least one given                                                      */
  const double* xdot_next_bar;      /* [n][3]                                                                            */
  const double* w_next_bar;         /* [n][3]                                                                            */
  const double* joint_q_next_bar;   /* [n][4][3]                                                                         */
  const double* joint_qdot_next_bar; /* [n][4][3]                                                                        */
  double* Rwb_bar;                  /* [n][9]    outputs: each optional, at least one given (flags counts)               */
  double *x_bar, *xdot_bar, *w_bar; /* [n][3] each                                                                       */
  double *joint_q_bar, *joint_qdot_bar, *joint_tau_bar; /* [n][4][3] each                                                */
  int32_t* flags;                   /* [n]: bit l singular J(q_l), bit 4 + l out of reach or singular J(qn_l)            */
  double leg_inertia[3];            /* kg m^2 (hip, thigh, calf), finite and > 0: the step's                             */
  double dt;                        /* seconds, finite, > 0: the step's                                                  */
} qc_leg_plant_adjoint_io;
/* struct_size set, pointers NULL, dt = 1/300, leg_inertia = 0 (the caller must give the step's). */
void qc_default_leg_plant_adjoint(qc_leg_plant_adjoint_io* io);
/* Asynchronous on `stream`, no host synchronisation (graph-capturable); n == 0 launches nothing and returns QC_OK.
 * QC_ERR_INVALID (message starting with "qc_leg_plant_step_adjoint_batch:", nothing launched) for a null handle or `io`, a wrong
 * struct_size, a dt or a leg_inertia entry that is not finite and > 0, no input cotangent at all, no output at all, a missing Rwb,
 * x, xdot, w, joint_q, joint_qdot or joint_tau, n beyond one launch, or a handle whose mass or Ib qc_plant_step_batch refuses. */
int qc_leg_plant_step_adjoint_batch(qc_handle* h, size_t n, const qc_leg_plant_adjoint_io* io, void* stream);

/* Differentiating the tick through a gait: the reverse pass of the SWING legs' PD torques, which qc_sensitivity_kin_batch leaves out.
 * With swing references (swing_pos, swing_vel) the tick commands, for every swing leg l and whatever the QP's status,
 *   p_b = Rwb^T pos_l - x (sic),  v_b = Rwb^T vel_l,  q_ref = IK(p_b),  qd = J(q_ref)^-1 v_b,
 *   tau_raw = kp o e + kd o (qd - joint_qdot_l) + kff,  e = wrapPI(wrap2PI(q_ref) - wrap2PI(joint_q_l)),
 * clamped by two compares to [tau_min, tau_max] (qc_set_kinematics holds the gains and the limits).  Given joint_tau_bar, the
 * cotangent on qc_batch_out.joint_tau, this writes per swing leg - tau_raw evaluated by the tick's own device function, so the
 * clamp mask is the forward pass's bit for bit -
 *   m_c = 1 where !(tau_raw_c < tau_min) && !(tau_raw_c > tau_max),  s = m o joint_tau_bar_l
 *   joint_q_bar_l = joint_q_bar_in_l - kp o s,  joint_qdot_bar_l = -kd o s          (the wrapped error has slope +1 in q_ref, -1 in q)
 *   gain_bar_l = (s o e, s o (qd - joint_qdot_l), s)                                nine numbers: kp, kd, kff
 *   g = J(q_ref)^-T (kd o s),  q_ref_bar = kp o s - (sum_r g_r d^2 FK_r / dq^2 (q_ref)) qd,  p_b_bar = J(q_ref)^-T q_ref_bar
 *                                                                                   (inside reach the IK inverts the FK)
 *   swing_pos_bar_l = Rwb p_b_bar,  swing_vel_bar_l = Rwb g
 * and per robot, summed over its swing legs in a fixed order,
 *   Rwb_bar[r][i] = Rwb_bar_in[r][i] + sum_l (pos_l,r p_b_bar_i + vel_l,r g_i)      ENTRYWISE, row-major: qc_sensitivity_rot_io's
 *   x_bar = x_bar_in - sum_l p_b_bar                                                (the body-frame subtraction as written)
 * A STANCE leg contributes nothing: its rows of the per-leg outputs are zero (joint_q_bar: joint_q_bar_in).  A missing `_in` counts
 * as zero.  Of `in` the call reads Rwb, x, joint_q, joint_qdot, swing_pos, swing_vel and the contact mask, resolved as
 * qc_sensitivity_kin_batch resolves it (`stance` bytes, else the phase rule on gait_phase as it is now, else all stance); `in` is
 * never written.
 * UNDEFINED GRADIENTS: `flags` bit l - swing leg l's reference is outside the smooth domain of the chain: the knee cosine d >= 1
 * (clamped) or d < -1, y^2 + z^2 - l1^2 < 0 (clamped), a target that is not finite, or det J(q_ref) outside the closed-form band
 * (the tick took the pseudo-inverse).  A flagged leg has NaN in its rows of the per-leg outputs and in the robot's Rwb_bar and
 * x_bar, whatever the mask.  Other non-finite inputs propagate.
 * NOT produced: the cotangents of the kinematic constants and of tau_min / tau_max; anything through swing_state's planner or the
 * gait clock (both refused); commander mode.
 * Each output may be the SAME array as its `_in`: every input of a robot is read before any of its outputs is written.  All
 * pointers are DEVICE pointers. */
typedef struct qc_sensitivity_swing_io {
  size_t struct_size;            /* = sizeof(qc_sensitivity_swing_io); checked                        */
  const double* joint_tau_bar;   /* [n][4][3] cotangent on qc_batch_out.joint_tau; required           */
  const double* joint_q_bar_in;  /* [n][4][3] added to joint_q_bar; optional                          */
  const double* Rwb_bar_in;      /* [n][9]    added to Rwb_bar; optional                              */
  const double* x_bar_in;        /* [n][3]    added to x_bar; optional                                */
  double* swing_pos_bar;         /* [n][4][3] OUT: each optional, at least one given (flags counts)   */
  double* swing_vel_bar;         /* [n][4][3]                                                         */
  double* joint_q_bar;           /* [n][4][3]                                                         */
  double* joint_qdot_bar;        /* [n][4][3]                                                         */
  double* gain_bar;              /* [n][4][9] kp, kd, kff of every leg                                */
  double* Rwb_bar;               /* [n][9]    entrywise, row-major                                    */
  double* x_bar;                 /* [n][3]                                                            */
  int32_t* flags;                /* [n]: bit l - swing leg l has no gradient                          */
} qc_sensitivity_swing_io;
/* struct_size set, pointers NULL. */
void qc_default_sensitivity_swing(qc_sensitivity_swing_io* io);
/* Asynchronous on `stream`, no host synchronisation (graph-capturable); n == 0 launches nothing and returns QC_OK.  No buffer is
 * kept on the handle.  QC_ERR_INVALID (message starting with "qc_sensitivity_swing_batch:", nothing launched) for a null handle,
 * `in` or `io`, a wrong struct_size, a swing_state or a gait_dt in `in`, no output requested, a missing joint_tau_bar, a missing
 * Rwb, x, joint_q, joint_qdot, swing_pos or swing_vel, or n beyond one launch. */
int qc_sensitivity_swing_batch(qc_handle* h, size_t n, const qc_batch_in* in, const qc_sensitivity_swing_io* io, void* stream);

/* The swing references as a launch of their own: what the tick does BEFORE the QP when qc_batch_in.swing_state is given, per robot
 * and in the tick's order, by the tick's own device functions - the values are the tick's bit for bit.
 *   1. clock  if in->gait_dt is given the four phases advance (phase += dt / (t_swing + t_stance), fmod 1) and are written back to
 *             in->gait_phase;
 *   2. mask   in->stance bytes, else the phase rule on the (advanced) phases with in->gait_duty or the handle's value;
 *   3. plan   leg l gets a new foothold on a stance -> swing edge, or whenever it swings on the first call (leg_state = -1):
 *             p_start_l = Rwb FK(joint_q_l) + x, p_final_l = the Raibert + LIP foothold (foot_planner.cpp:76-104).  If ANY leg is
 *             replanned, has_traj of every other leg is cleared (trajectory.cpp:308-344), else it is kept; leg_state = the mask;
 *   4. track  swing leg with a trajectory: swing_pos_l, swing_vel_l = the sextic through p_start_l, the centre ((p_start_l +
 *             p_final_l) / 2 in x, y; swing_height in z) and p_final_l at the leg's phase, WORLD frame - the arrays qc_control_batch
 *             takes as qc_batch_in.swing_pos / swing_vel.  A stance leg and a swing leg without a trajectory get zeros.
 * So qc_control_batch with swing_state and gait_dt equals this call with the same gait_dt followed by qc_control_batch with the
 * returned swing_pos / swing_vel and the phases it left (no gait_dt): records, phases, joint_tau, grf_body and status.
 * Of `in` it reads Rwb, x, xdot, w, xdot_d, joint_q, gait_phase and swing_state (IN/OUT) - all required - and the optional stance,
 * gait_duty and gait_dt; the other members are ignored, except that `feet` without joint_q and a swing_pos / swing_vel are refused.
 * In commander mode qc_commander_step_batch comes first: its xdot_d is the one this call takes.  All pointers are DEVICE pointers. */
typedef struct qc_swing_reference_io {
  size_t struct_size;  /* = sizeof(qc_swing_reference_io); checked                           */
  double* swing_pos;   /* [n][4][3] OUT: each optional, at least one given                    */
  double* swing_vel;   /* [n][4][3]                                                           */
  uint8_t* planned;    /* [n]: bit l - leg l was replanned by this call                       */
} qc_swing_reference_io;
/* struct_size set, pointers NULL. */
void qc_default_swing_reference(qc_swing_reference_io* io);
/* Asynchronous on `stream`, no host synchronisation (graph-capturable); n == 0 launches nothing and returns QC_OK.  QC_ERR_INVALID
 * (message starting with "qc_swing_reference_batch:", nothing launched) for a null handle, `in` or `io`, a wrong struct_size, a
 * swing_pos or swing_vel in `in`, `feet` without joint_q, gait_dt together with stance, no output requested, a missing Rwb, x, xdot, w,
 * xdot_d, joint_q, gait_phase or swing_state, or n beyond one launch. */
int qc_swing_reference_batch(qc_handle* h, size_t n, const qc_batch_in* in, const qc_swing_reference_io* io, void* stream);

/* The reverse pass of qc_swing_reference_batch.  The forward launch saves nothing: pass the same `in` with gait_phase AS THE FORWARD
 * CALL LEFT IT (gait_dt is refused: no clock is advanced here) and `state_before`, a copy of the qc_swing_state records from BEFORE the
 * forward call - the plan decision is recomputed from its leg_state / has_traj and the contact mask.  With (h, h') the sextic's basis
 * functions and their derivatives at leg l's clamped trajectory time (zero if the leg is in stance or has no trajectory after the
 * call), per leg
 *   a_r = (h0 + h2 / 2) swing_pos_bar_r + (h0' + h2' / 2) swing_vel_bar_r,  c_r likewise with h1, h1'      r = 0, 1
 *   a_2 = h0 swing_pos_bar_2 + h0' swing_vel_bar_2,                         c_2 likewise                    (the centre's z is a constant)
 *   A = a + p_start_next_bar_l,  C = c + p_final_next_bar_l                 the total on the record after the call
 *   leg NOT replanned:  p_start_bar_l = A,  p_final_bar_l = C               (the record passed through)
 *   leg replanned:      p_start_bar_l = p_final_bar_l = 0 (overwritten);  C_2 := 0 (the foothold's z is 0);  with p = FK(joint_q_l),
 *                       r = Rwb p, half = t_stance / 2, k = planner_k, lip = sqrt(x_z / 9.81) / 2, hip = planner_hip[l]:
 *     x_bar += A + C,  x_bar[2] += 0.25 / (9.81 sqrt(x_z / 9.81)) <C, xdot>,  xdot_bar += (half + k + lip) C,  xdot_d_bar += -k C,
 *     w_bar += half (r x C),  r_bar = A + half (C x w),  Rwb_bar += r_bar p^T + C hip^T     ENTRYWISE, row-major: qc_sensitivity_rot_io's
 *     joint_q_bar_l += J(joint_q_l)^T Rwb^T r_bar
 * summed over the legs in the order 0, 1, 2, 3 on top of the `_in` arrays (a missing one counts as zero, as does a missing cotangent).
 * Of `in` it reads Rwb, x, xdot, w, joint_q, gait_phase - required - and the optional stance and gait_duty; `in` is never written.
 * UNDEFINED GRADIENT: `flags` bit l - leg l is replanned and x_z is not finite and > 0: the LIP square root has no derivative there;
 * every output row of that robot is NaN.  Other non-finite inputs propagate; nothing is clamped.
 * NOT produced: a cotangent of the phases, of gait_dt, of the gait's periods, of swing_height, planner_k or the kinematic constants -
 * the clock and the contact mask are held, as in qc_leg_plant_step_adjoint_batch.  In commander mode xdot_d_bar goes on to
 * qc_commander_step_adjoint_batch.
 * Each of Rwb_bar, x_bar, xdot_bar, w_bar and joint_q_bar may be the SAME array as its `_in`, and p_start_bar / p_final_bar the same
 * arrays as p_start_next_bar / p_final_next_bar: every input of a robot is read before any of its outputs is written.  All pointers
 * are DEVICE pointers. */
typedef struct qc_swing_reference_adjoint_io {
  size_t struct_size;                         /* = sizeof(qc_swing_reference_adjoint_io); checked                    */
  const struct qc_swing_state* state_before;  /* [n] the records before the forward call; required                   */
  const double* swing_pos_bar;                /* [n][4][3] cotangents: each optional, at least one given             */
  const double* swing_vel_bar;                /* [n][4][3]                                                           */
  const double* p_start_next_bar;             /* [n][12]   on the record after the call                              */
  const double* p_final_next_bar;             /* [n][12]                                                             */
  const double* Rwb_bar_in;                   /* [n][9]    added to the output of that name; each optional           */
  const double* x_bar_in;                     /* [n][3]                                                              */
  const double* xdot_bar_in;                  /* [n][3]                                                              */
  const double* w_bar_in;                     /* [n][3]                                                              */
  const double* joint_q_bar_in;               /* [n][4][3]                                                           */
  double* Rwb_bar;                            /* [n][9]    OUT: each optional, at least one given (flags counts)     */
  double* x_bar;                              /* [n][3]                                                              */
  double* xdot_bar;                           /* [n][3]                                                              */
  double* w_bar;                              /* [n][3]                                                              */
  double* xdot_d_bar;                         /* [n][3]                                                              */
  double* joint_q_bar;                        /* [n][4][3]                                                           */
  double* p_start_bar;                        /* [n][12]   on the record before the call                             */
  double* p_final_bar;                        /* [n][12]                                                             */
  int32_t* flags;                             /* [n]: bit l - replanned leg l has no gradient                        */
} qc_swing_reference_adjoint_io;
/* struct_size set, pointers NULL. */
void qc_default_swing_reference_adjoint(qc_swing_reference_adjoint_io* io);
/* Asynchronous on `stream`, no host synchronisation (graph-capturable); n == 0 launches nothing and returns QC_OK.  QC_ERR_INVALID
 * (message starting with "qc_swing_reference_adjoint_batch:", nothing launched) for a null handle, `in` or `io`, a wrong struct_size,
 * a gait_dt, swing_pos or swing_vel in `in`, `feet` without joint_q, no cotangent given, no output requested, a missing state_before,
 * a missing Rwb, x, xdot, w, joint_q or gait_phase, or n beyond one launch. */
int qc_swing_reference_adjoint_batch(qc_handle* h, size_t n, const qc_batch_in* in, const qc_swing_reference_adjoint_io* io, void* stream);

/* The commander step as a launch of its own: what qc_tick_batch does FIRST for every robot (steps 1-3 of "Commander mode" above), by
 * the tick's own device function - the values are the tick's bit for bit.  `cmd` is qc_tick_batch's: twist, fresh, state (IN/OUT,
 * updated in place exactly as the tick updates it), stand_height, stand_tol, cmd_dt.  Every state of the record is handled: a fresh
 * command or none; not standing; standing but not running (gait_running is set, nothing else); running with or without a pending
 * command.  Optionally written: the desired state the tick would feed the QP THIS tick - the record's own where no command was
 * applied - `run` (the gait runs this tick: gait_running was set before the call and standing is set after it) and
 * `applied` (a command was applied by this call).
 * CONTRACT: for a batch in which every robot has standing and gait_running set, qc_tick_batch equals this call followed by
 * qc_control_batch on the same `in` with the four returned arrays as Rwb_d / x_d / xdot_d / w_d (swing_state and gait_dt unchanged) in
 * joint_tau, grf_body, status, phases, swing records and commander records, bit for bit.  For ANY batch the commander records after
 * this call equal those after qc_tick_batch, bit for bit.
 * Of `in` it reads Rwb and x only.  All pointers are DEVICE pointers. */
typedef struct qc_commander_step_io {
  size_t struct_size; /* = sizeof(qc_commander_step_io); checked                                   */
  double* Rwb_d;      /* [n][9] OUT, row-major: each optional (the records are always updated)     */
  double* x_d;        /* [n][3]                                                                    */
  double* xdot_d;     /* [n][3]                                                                    */
  double* w_d;        /* [n][3]                                                                    */
  uint8_t* run;       /* [n]: 1 - the gait runs this tick                                          */
  uint8_t* applied;   /* [n]: 1 - a command was applied by this call                               */
} qc_commander_step_io;
/* struct_size set, pointers NULL. */
void qc_default_commander_step(qc_commander_step_io* io);
/* Asynchronous on `stream`, no host synchronisation (graph-capturable); n == 0 launches nothing and returns QC_OK.  QC_ERR_INVALID
 * (message starting with "qc_commander_step_batch:", nothing launched) for a null handle, `in`, `cmd` or `io`, a wrong struct_size of
 * either record, a missing cmd->state, Rwb or x, `fresh` without `twist`, a stand_height, stand_tol (>= 0) or cmd_dt that is not
 * finite, or n beyond one launch. */
int qc_commander_step_batch(qc_handle* h, size_t n, const qc_batch_in* in, const qc_command_in* cmd, const qc_commander_step_io* io, void* stream);

/* The reverse pass of qc_commander_step_batch.  The forward launch saves nothing: pass the same Rwb, x (`in`), twist, fresh and the
 * three scalars (`cmd`; cmd->state is not read) and `state_before`, a copy of the qc_commander_state records from BEFORE the forward
 * call.  The branch decisions (fresh, standing, running, pending, applied) are recomputed from those and held.
 * Cotangents in (a missing one counts as zero): G = Rwb_d_bar (ENTRYWISE, row-major: qc_sensitivity_rot_io's layout), a = x_d_bar,
 * b = xdot_d_bar, c = w_d_bar - on the four arrays the forward call returns - and Vb_next_bar, on the held command AFTER the call.
 *   command source  vb = fresh ? twist : Vb.  Its total cotangent vb_bar is Vb_next_bar (a fresh twist is stored as Vb, a held one
 *                   stays) plus the applied terms below.  fresh: twist_bar = vb_bar, Vb_bar = 0.  held: Vb_bar = vb_bar, twist_bar = 0.
 *   NOT applied     Rwb_d_prev_bar, x_d_prev_bar, xdot_d_prev_bar, w_d_prev_bar = G, a, b, c: the record passed through.  Nothing reaches
 *                   Rwb_bar, x_bar (they equal their `_in`) or vb.
 *   applied         the four _prev_bar are zero: the record was overwritten.  The forward function, with v = vb[0:3], om = vb[3:6],
 *                   d = cmd_dt om, Rb = Exp(d), t = cmd_dt Rb v, Y = Rz(yaw), (cy, sy) = (R00, R10) / h, h = hypot(R00, R10):
 *                     Rwb_d = Y Rb,  x_d = (x0 + (Y t)0, x1 + (Y t)1, stand_height),  xdot_d = Rwb^T (v - x x om),  w_d = Rwb^T om
 *                   is reversed exactly: a_2 is dropped (the height is a constant), and with u = v - x x om, ub = Rwb b, tb = Y^T (a_0, a_1, 0),
 *                   M = Y^T G + cmd_dt tb v^T, wv = axial(M Rb^T), d_bar = Jl(d)^T wv (Jl: the left Jacobian of Exp):
 *                     v_bar = ub + cmd_dt Rb^T tb,  om_bar = Rwb c + x x ub + cmd_dt d_bar,  x_bar += ub x om + (a_0, a_1, 0),
 *                     Rwb_bar[i][k] += u_i b_k + om_i c_k (every entry, from the two Rwb^T products), and entries 0 and 3 get the yaw
 *                     normalisation: with cy_bar, sy_bar the cotangents of (cy, sy) from Y t and Y Rb and q = cy_bar sy - sy_bar cy,
 *                     Rwb_bar[0] += sy q / h,  Rwb_bar[3] -= cy q / h.
 *   small angle     |d| < 1e-12, where the forward pass takes Rb = I and t = cmd_dt v: the SMOOTH function is differentiated - Exp and Jl
 *                   by their own formulas down to d = 0, where delta Rb = [delta d]x, delta t = cmd_dt [delta d]x v (d_bar = wv) - not
 *                   the branch as written, whose derivative in om is zero: a twist with zero angular rate is where an optimisation
 *                   starts, and a yaw-rate command must not get a silently zero gradient there (qc_sensitivity_rot_batch's
 *                   "smooth limit at zero error").
 * Rwb_bar and x_bar are added on top of Rwb_bar_in / x_bar_in (a missing one counts as zero).
 * UNDEFINED GRADIENT: `flags` bit 0 - a command is applied at the gimbal-lock branch (h == 0, or h not finite and below 1e300, where
 * the forward pass takes yaw 0); every output row of that robot is NaN.  Other non-finite inputs propagate; nothing is clamped.
 * NOT produced: cotangents of stand_height, stand_tol, cmd_dt; the flags and latches are held.
 * Each of Rwb_bar, x_bar may be the SAME array as its `_in`; Vb_bar the same as Vb_next_bar; the four _prev_bar the same as the four
 * desired-state cotangents: every input of a robot is read before any of its outputs is written.  All pointers are DEVICE pointers. */
typedef struct qc_commander_step_adjoint_io {
  size_t struct_size;                             /* = sizeof(qc_commander_step_adjoint_io); checked                 */
  const struct qc_commander_state* state_before;  /* [n] the records before the forward call; required               */
  const double* Rwb_d_bar;                        /* [n][9] cotangents: each optional, at least one given            */
  const double* x_d_bar;                          /* [n][3]                                                          */
  const double* xdot_d_bar;                       /* [n][3]                                                          */
  const double* w_d_bar;                          /* [n][3]                                                          */
  const double* Vb_next_bar;                      /* [n][6] on the held command after the call                       */
  const double* Rwb_bar_in;                       /* [n][9] added to the output of that name; each optional          */
  const double* x_bar_in;                         /* [n][3]                                                          */
  double* twist_bar;                              /* [n][6] OUT: each optional, at least one given (flags counts)    */
  double* Vb_bar;                                 /* [n][6] on the held command before the call                      */
  double* Rwb_bar;                                /* [n][9]                                                          */
  double* x_bar;                                  /* [n][3]                                                          */
  double* Rwb_d_prev_bar;                         /* [n][9] on the record's desired state before the call            */
  double* x_d_prev_bar;                           /* [n][3]                                                          */
  double* xdot_d_prev_bar;                        /* [n][3]                                                          */
  double* w_d_prev_bar;                           /* [n][3]                                                          */
  int32_t* flags;                                 /* [n]: bit 0 - applied at gimbal lock, no gradient                */
} qc_commander_step_adjoint_io;
/* struct_size set, pointers NULL. */
void qc_default_commander_step_adjoint(qc_commander_step_adjoint_io* io);
/* Asynchronous on `stream`, no host synchronisation (graph-capturable); n == 0 launches nothing and returns QC_OK.  QC_ERR_INVALID
 * (message starting with "qc_commander_step_adjoint_batch:", nothing launched) for a null handle, `in`, `cmd` or `io`, a wrong
 * struct_size of either record, no cotangent given, no output requested, a missing state_before, Rwb or x, `fresh` without `twist`,
 * a stand_height, stand_tol (>= 0) or cmd_dt that is not finite, or n beyond one launch. */
int qc_commander_step_adjoint_batch(qc_handle* h, size_t n, const qc_batch_in* in, const qc_command_in* cmd, const qc_commander_step_adjoint_io* io, void* stream);

/* The virtual support polygon (SupportPolygon::position, trajectory.cpp:73-147): from the scheduled gait, the x, y position at which
 * the COM should be held.  Per robot, in the reference's evaluation order, with the legs RL, FL, RR, FR = 0, 1, 2, 3 and the
 * neighbours (minus, plus) of trajectory.cpp:75-78 - RL: (FL, RR), FL: (FR, RL), FR: (RR, FL), RR: (RL, FR):
 *   1. weight  with phi the leg's RAW gait phase (gait_map.second: not a sub-phase of the stance or of the swing) and
 *              (c0, cf, s0, sf) = schedule[l] = LegScheduledPhases' (stance_start, stance_end, swing_start, swing_end) - which are
 *              the WIDTHS (sigma) of the erf ramps, whatever their names say:
 *                stance leg  w = 0.5 (erf(phi / (c0 sqrt2 + 1e-12)) + erf((1 - phi) / (cf sqrt2 + 1e-12)))
 *                swing leg   w = 0.5 (2 + erf(-phi / (s0 sqrt2 + 1e-12)) + erf((phi - 1) / (sf sqrt2 + 1e-12)))
 *   2. points  P = the foot's x, y; zm = P w + P_minus (1 - w), zp = P w + P_plus (1 - w);
 *              v = (1 / (w + w_minus + w_plus)) (w P + w_minus zm + w_plus zp)
 *   3. mean    com_xy = (v_FL + v_FR + v_RL + v_RR) / 4, summed in that order (the reference's std::map)
 * Of `in` it reads the feet - joint_q through the device forward kinematics if given, else `feet` (allowed here without joint_q) -
 * gait_phase (required, never written) and the contact mask as every entry point resolves it: `stance` bytes, else the phase rule
 * with gait_duty or the handle's value.  gait_dt, swing_state, swing_pos and swing_vel are refused; the rest is ignored unless
 * `world` is set: then Rwb and x are required and P is taken of Rwb p + x, so com_xy is a WORLD-frame x, y that can be written
 * straight into x_d[:, :2].
 * `flags` bit l: the denominator of leg l's point is zero or not finite - the reference's 0/0.  The arithmetic is reproduced (the
 * robot's com_xy is NaN); nothing is clamped.  All pointers are DEVICE pointers. */
typedef struct qc_support_polygon_io {
  size_t struct_size;      /* = sizeof(qc_support_polygon_io); checked                                          */
  const double* schedule;  /* [n][4][4] the widths (c0, cf, s0, sf) per leg; required                            */
  int32_t schedule_shared; /* nonzero: `schedule` is ONE [4][4] block read by every robot                        */
  int32_t world;           /* nonzero: the polygon of Rwb p + x (in->Rwb and in->x required)                     */
  double* com_xy;          /* [n][2] OUT: each optional, at least one given                                      */
  double* weights;         /* [n][4]                                                                             */
  int32_t* flags;          /* [n]: bit l - leg l's point is 0/0                                                  */
} qc_support_polygon_io;
/* struct_size set, the rest zero. */
void qc_default_support_polygon(qc_support_polygon_io* io);
/* Asynchronous on `stream`, no host synchronisation (graph-capturable); n == 0 launches nothing and returns QC_OK.  QC_ERR_INVALID
 * (message starting with "qc_support_polygon_batch:", nothing launched) for a null handle, `in` or `io`, a wrong struct_size, a
 * gait_dt, swing_state, swing_pos or swing_vel in `in`, no output requested, a missing schedule, gait_phase, feet / joint_q, `world`
 * without Rwb or x, or n beyond one launch. */
int qc_support_polygon_batch(qc_handle* h, size_t n, const qc_batch_in* in, const qc_support_polygon_io* io, void* stream);

/* The reverse pass of qc_support_polygon_batch.  The forward launch saves nothing: pass the same `in`, schedule, schedule_shared and
 * world.  With g = com_xy_bar, per leg l in the order 0, 1, 2, 3 (m, p its minus and plus neighbours, D_l = w_l + w_m + w_p):
 *   Nb = (g / 4) / D_l,  Db = -<g / 4, v_l> / D_l
 *   wb_l += Db + <Nb, P_l> + w_m <Nb, P_l - P_m> + w_p <Nb, P_l - P_p>,  wb_m += Db + <Nb, zm_l>,  wb_p += Db + <Nb, zp_l>
 *   Pb_l += (w_l + w_l w_m + w_l w_p) Nb,  Pb_m += w_m (1 - w_l) Nb,  Pb_p += w_p (1 - w_l) Nb
 * then per leg, with a1, a2 the two erf arguments, d1, d2 their denominators, e_i = exp(-a_i^2) / sqrt(pi), sgn = +1 (stance), -1 (swing):
 *   phase_bar_l = wb_l sgn (e1 / d1 - e2 / d2);  the two widths the leg's branch reads get -wb_l e_i a_i sqrt2 / d_i, the other two 0
 *   body mode   feet_bar_l = (Pb_l, 0)
 *   world mode  feet_bar_l = Rwb^T (Pb_l, 0) - BODY frame, what qc_sensitivity_kin_batch carries on to joint_q_bar -
 *               Rwb_bar += (Pb_l, 0) p_l^T (ENTRYWISE, row-major: qc_sensitivity_rot_io's layout),  x_bar += (Pb_l, 0)  (z = 0)
 * on top of the `_in` arrays (a missing one counts as zero).  In body mode Rwb_bar and x_bar equal their `_in`.
 * The contact mask is HELD: a phase exactly on the stance / swing boundary gets the gradient of the branch the forward pass took.
 * schedule_bar is [n][4][4], one block per robot, with a shared schedule too: it is NOT summed over the batch.
 * A robot flagged by the forward rule (`flags`, as above) gets NaN in every output row.
 * Each output may be the SAME array as its `_in`: every input of a robot is read before any of its outputs is written.  All
 * pointers are DEVICE pointers. */
typedef struct qc_support_polygon_adjoint_io {
  size_t struct_size;            /* = sizeof(qc_support_polygon_adjoint_io); checked                             */
  const double* schedule;        /* as the forward call's                                                        */
  int32_t schedule_shared;
  int32_t world;
  const double* com_xy_bar;      /* [n][2] the cotangent; required                                               */
  const double* feet_bar_in;     /* [n][4][3] added to the output of that name; each optional                    */
  const double* Rwb_bar_in;      /* [n][9]                                                                       */
  const double* x_bar_in;        /* [n][3]                                                                       */
  const double* phase_bar_in;    /* [n][4]                                                                       */
  const double* schedule_bar_in; /* [n][4][4]                                                                    */
  double* feet_bar;              /* [n][4][3] OUT, body frame: each optional, at least one given (flags counts)  */
  double* Rwb_bar;               /* [n][9]                                                                       */
  double* x_bar;                 /* [n][3]                                                                       */
  double* phase_bar;             /* [n][4]                                                                       */
  double* schedule_bar;          /* [n][4][4]                                                                    */
  int32_t* flags;                /* [n]: bit l - leg l's point is 0/0, no gradient                               */
} qc_support_polygon_adjoint_io;
/* struct_size set, the rest zero. */
void qc_default_support_polygon_adjoint(qc_support_polygon_adjoint_io* io);
/* Asynchronous on `stream`, no host synchronisation (graph-capturable); n == 0 launches nothing and returns QC_OK.  QC_ERR_INVALID
 * (message starting with "qc_support_polygon_adjoint_batch:", nothing launched) for a null handle, `in` or `io`, a wrong
 * struct_size, a gait_dt, swing_state, swing_pos or swing_vel in `in`, no output requested, a missing com_xy_bar, schedule,
 * gait_phase, feet / joint_q, `world` without Rwb or x, or n beyond one launch. */
int qc_support_polygon_adjoint_batch(qc_handle* h, size_t n, const qc_batch_in* in, const qc_support_polygon_adjoint_io* io, void* stream);

/* The desired COM position of a step from the virtual support polygon: one launch in front of the tick makes the x_d it tracks.
 * Of `in` it reads what qc_support_polygon_batch reads with `world` set - gait_phase, joint_q (device forward kinematics) or feet,
 * the contact mask (`stance` bytes, else the phase rule), Rwb and x (both required) - and refuses the same batches (gait_dt,
 * swing_state, swing_pos, swing_vel).  With P_l the x, y of Rwb p_l + x and com_xy the polygon's value, by the polygon's own device
 * functions (com_xy equals qc_support_polygon_batch's bit for bit):
 *   QC_COM_REPLACE  x_d_out = (com_xy, x_d_in.z);  gain is ignored
 *   QC_COM_OFFSET   x_d_out = x_d_in + gain (com_xy - centroid_xy, 0),  centroid_xy = (((P_FL + P_FR) + P_RL) + P_RR) / 4
 * With all four weights 1, com_xy = centroid_xy in exact arithmetic: the offset is the lean alone, and an x_d that tracks a twist
 * is not dragged to the feet.  z is copied.  `flags` as the polygon's (bit l: the reference's 0/0 at leg l's point); a flagged
 * robot gets NaN in x_d_out's x and y, com_xy is what the reference's arithmetic gives.  x_d_out may be the SAME array as x_d_in:
 * every input of a robot is read before any of its outputs is written.  All pointers are DEVICE pointers. */
enum { QC_COM_REPLACE = 0, QC_COM_OFFSET = 1 };
typedef struct qc_com_reference_io {
  size_t struct_size;      /* = sizeof(qc_com_reference_io); checked                                              */
  const double* schedule;  /* [n][4][4] the widths (c0, cf, s0, sf) per leg; required                            */
  int32_t schedule_shared; /* nonzero: `schedule` is ONE [4][4] block read by every robot                        */
  int32_t mode;            /* QC_COM_REPLACE or QC_COM_OFFSET                                                    */
  double gain;             /* QC_COM_OFFSET's factor, finite; default 1                                          */
  const double* x_d_in;    /* [n][3]; required                                                                   */
  double* x_d_out;         /* [n][3] OUT; required, may be x_d_in                                                */
  double* com_xy;          /* [n][2] OUT, optional: the polygon's value                                          */
  int32_t* flags;          /* [n] OUT, optional                                                                  */
} qc_com_reference_io;
/* struct_size set, mode = QC_COM_REPLACE, gain = 1, the rest zero. */
void qc_default_com_reference(qc_com_reference_io* io);
/* Asynchronous on `stream`, no host synchronisation (graph-capturable); n == 0 launches nothing and returns QC_OK.  QC_ERR_INVALID
 * (message starting with "qc_com_reference_batch:", nothing launched) for a null handle, `in` or `io`, a wrong struct_size, a
 * gait_dt, swing_state, swing_pos or swing_vel in `in`, an unknown mode, a gain that is not finite, a missing x_d_out, x_d_in,
 * schedule, gait_phase, feet / joint_q, Rwb or x, or n beyond one launch. */
int qc_com_reference_batch(qc_handle* h, size_t n, const qc_batch_in* in, const qc_com_reference_io* io, void* stream);

/* The reverse pass of qc_com_reference_batch.  The forward launch saves nothing: pass the same `in`, schedule, schedule_shared,
 * mode and gain.  With o = x_d_out_bar:
 *   QC_COM_REPLACE  x_d_in_bar = (0, 0, o.z);  the polygon's reverse pass (qc_support_polygon_adjoint_batch, world mode) from
 *                   com_xy_bar = o.xy
 *   QC_COM_OFFSET   x_d_in_bar = o;  the polygon's reverse pass from com_xy_bar = gain o.xy, and the centroid adds
 *                   -gain o.xy / 4 to every Pb_l before the points are carried on to feet_bar, Rwb_bar and x_bar
 * feet_bar (BODY frame), Rwb_bar (entrywise), x_bar, phase_bar and schedule_bar ([n][4][4], one block per robot) go on top of
 * their `_in` arrays (a missing one counts as zero), each of which may be its own output, and x_d_in_bar may be x_d_out_bar.
 * `gain` gets NO cotangent, nor do the contact mask (held) and the mode.  A robot flagged by the forward rule gets NaN in every
 * output row, x_d_in_bar's included.
 * schedule_bar_sum [16]: the schedule_bar rows as they are (or would be) stored - the `_in` rows included - summed over the batch
 * WITHOUT atomics, in an order that depends on n alone: the result is bit-reproducible and the same with and without the rows.  With
 * B = min(ceil(n / 64), 1024) and every sum starting from 0.0:
 *   1. partial[b], b < B: for r = 0, 1, ... while (b + r B) 64 < n, for j = 0 .. 63 while i = (b + r B) 64 + j < n: partial[b] += row[i]
 *   2. group[w], w < 16: for p = w, w + 16, w + 32, ... < B: group[w] += partial[p]
 *   3. schedule_bar_sum = (..((group[0] + group[1]) + group[2]) .. + group[15])
 * entry by entry.  A flagged robot makes the sum NaN.  It is allowed with a per-robot schedule too: it is then the sum of the rows,
 * nothing more.  The partials live in a buffer of the handle: two calls that ask for the sum must not overlap on different streams.
 * All pointers are DEVICE pointers. */
typedef struct qc_com_reference_adjoint_io {
  size_t struct_size;            /* = sizeof(qc_com_reference_adjoint_io); checked                               */
  const double* schedule;        /* as the forward call's                                                        */
  int32_t schedule_shared;
  int32_t mode;
  double gain;
  const double* x_d_out_bar;     /* [n][3] the cotangent; required                                               */
  const double* feet_bar_in;     /* [n][4][3] added to the output of that name; each optional                    */
  const double* Rwb_bar_in;      /* [n][9]                                                                       */
  const double* x_bar_in;        /* [n][3]                                                                       */
  const double* phase_bar_in;    /* [n][4]                                                                       */
  const double* schedule_bar_in; /* [n][4][4]                                                                    */
  double* x_d_in_bar;            /* [n][3] OUT: each optional, at least one given (flags counts); may be x_d_out_bar */
  double* feet_bar;              /* [n][4][3], body frame                                                        */
  double* Rwb_bar;               /* [n][9]                                                                       */
  double* x_bar;                 /* [n][3]                                                                       */
  double* phase_bar;             /* [n][4]                                                                       */
  double* schedule_bar;          /* [n][4][4]                                                                    */
  double* schedule_bar_sum;      /* [16]: the rows summed over the batch in the fixed order above                */
  int32_t* flags;                /* [n]: bit l - leg l's point is 0/0, no gradient                               */
} qc_com_reference_adjoint_io;
/* struct_size set, mode = QC_COM_REPLACE, gain = 1, the rest zero. */
void qc_default_com_reference_adjoint(qc_com_reference_adjoint_io* io);
/* Asynchronous on `stream`, no host synchronisation (graph-capturable); n == 0 launches nothing, writes nothing (schedule_bar_sum
 * is left as it is) and returns QC_OK.  QC_ERR_INVALID (message starting with "qc_com_reference_adjoint_batch:", nothing
 * launched) for a null handle, `in` or `io`, a wrong struct_size, a gait_dt, swing_state, swing_pos or swing_vel in `in`, an
 * unknown mode, a gain that is not finite, no output requested, a missing x_d_out_bar, schedule, gait_phase, feet / joint_q, Rwb or
 * x, or n beyond one launch. */
int qc_com_reference_adjoint_batch(qc_handle* h, size_t n, const qc_batch_in* in, const qc_com_reference_adjoint_io* io, void* stream);

#ifdef __cplusplus
}
#endif

/* The constructor every C / C++ caller uses (see qc_create_abi above): the ABI guard travels with it. */
static inline int qc_create(const qc_params* params, int device, qc_handle** out) {
  return qc_create_abi(params, device, out, QC_ABI_VERSION, sizeof(qc_params), sizeof(qc_batch_in), sizeof(qc_batch_out));
}
#endif /* QC_BALANCE_H */
