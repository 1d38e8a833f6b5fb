/* qc_tangent.h - forward mode of the balance QP: qc_tangent_batch pushes K tangents on the inputs of a solved batch through the
 * QP on its active face and returns the tangents of the forces.  A header beside qc_balance.h: its functions live in the same
 * libqc_balance.so, QC_ABI_VERSION and the records of qc_balance.h are untouched.
 *
 * Per robot the solve minimises (A f - b)^T S (A f - b) + f^T W f over the world-frame forces f under the pyramid rows described
 * at qc_certify_batch; H = 2 (A^T S A + W), g = 2 (A^T S (A f - b) + W f).  The call takes the SAME qc_batch_in the solve read
 * (contact mask resolved as qc_certify_batch resolves it; gait_dt and the swing arrays are ignored, `in` is never written) and the
 * forces.  The face is exactly qc_sensitivity_batch's: qc_certify_batch's codes at act_tol, coordinates pinned, tied or free; a
 * code 3 on any axis of a foot pins the whole foot and sets bit 0 of `flags` (the derivative is one-sided there).
 *
 * Per direction, with f_i = -Rwb grf_body_i, v = S (A f - b), delta / delta_d the rotation tangents (world-frame left tangents:
 * Rwb <- exp([delta]x) Rwb, Rwb_d <- exp([delta_d]x) Rwb_d):
 *   dp_i = feet_tan_i + J(q_i) joint_q_tan_i            the body-frame foot (J: the leg Jacobian of the handle's kinematic model)
 *   dr_i = delta x r_i + Rwb dp_i                       the lever arm r_i = Rwb p_i
 *   db   = the forward derivative of the PD law, line by line as the library evaluates it (the kff lines on xdot_d[0], xdot_d[1]
 *          and w_d included): b_lin = m (kp_p (x_d - x) + kd_p (xdot_d - xdot) + ...), b_ang = Iw al + w_d x (Iw w_d) with
 *          Iw = Rwb Ib Rwb^T, dIw = [delta]x Iw - Iw [delta]x, al = kp_w e + kd_w (w_d - w) + ..., and the rotation error
 *          e = log(Rwb_d Rwb^T) differentiated along dRe = [delta_d]x Re - Re [delta]x through the library's Eigen-convention log on
 *          the branch the evaluation took (at Re = I: the smooth limit, as in qc_sensitivity_rot_batch)
 *   dg_i = 2 (v_ang x dr_i + A_i^T S (dA f - db)),  dA f = (0; sum_i dr_i x f_i)      the gradient's tangent at fixed f
 *   df   = -Z (Z^T H Z)^-1 Z^T dg                       the solve on the face (factorised once per robot, substituted K times)
 *   grf_tan_i = -Rwb^T df_i + Rwb^T (delta x f_i),  b_tan = db.
 * With unit seeds the K outputs are K columns of the Jacobian d grf_body / d (inputs); <grf_bar, grf_tan> equals the pairing of
 * the tangents with the cotangents of qc_sensitivity_batch and qc_sensitivity_rot_batch (Rwb_rot_bar, Rwb_d_rot_bar).
 *
 * The reduced system is the fixed 12x12 LDL^T of qc_sensitivity_batch; a pivot that is not positive and finite sets bit 1 of
 * `flags` and every grf_tan and b_tan of that robot, in all K directions, is NaN.  A failed robot (all-zero forces) gets grf_tan = 0
 * exactly, and so does a robot with no stance foot whose forces are zero, as the solve writes them: the face is empty, and the
 * output transform's own term Rwb^T (delta x f_i) is still evaluated on the forces given.  Non-finite inputs propagate as NaN;
 * nothing is clamped.
 *
 * OUT OF SCOPE: entrywise (nine-number) rotation tangents - the rotations move along the left tangents above only; tangents of
 * the handle's parameters in THIS call (mu, fzmin, fzmax, the weights, the gains, mass, Ib: qc_param_tangent_batch, at the end of
 * the header, adds them in place on grf_tan; the kinematic model has no tangent); tangents through the swing
 * pipeline (the swing legs' PD torques and the planner's references have their own calls below; the gait clock is held); weak activity (a row whose multiplier is about 0
 * is on the face like any other); commander mode in THIS call (the desired state must be in `in`: qc_commander_step_tangent_batch,
 * below, gives its tangents); a jvp on the torch.autograd.Functions of the Python package.
 *
 * The rigid-body plant step has its forward mode below, qc_plant_step_tangent_batch: with it the two calls chain, step after step,
 * into the tangent of a closed-loop rollout.  The loop around the complete tick - joint_q -> FK -> QP -> clamped J^T -> joint_tau ->
 * legged plant - chains qc_tangent_batch (joint_q_tan), qc_torque_tangent_batch, for a batch with swing references
 * qc_swing_torque_tangent_batch in place behind it, and qc_leg_plant_step_tangent_batch, all below.  With swing_state the references
 * themselves move: qc_swing_reference_tangent_batch is the forward mode of the planner and the trajectory.  The two stages a rollout
 * is steered through close the header: qc_commander_step_tangent_batch (the twist command -> the desired state) and
 * qc_com_reference_tangent_batch (the schedule of the lean -> x_d).  With them every differentiable stage has both modes in the
 * state; qc_param_tangent_batch, the last call of the header, is the QP's forward mode in the handle's parameters. */
#ifndef QC_TANGENT_H
#define QC_TANGENT_H

#include "qc_balance.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct qc_tangent_io {
  size_t struct_size;            /* = sizeof(qc_tangent_io); checked                                                  */
  const double* grf_body;        /* [n][4][3] qc_batch_out.grf_body                                                   */
  double act_tol;                /* as qc_sensitivity_io.act_tol: finite, >= 0                                        */
  size_t n_dir;                  /* K >= 1 directions per launch                                                      */
  /* tangents, direction-major: direction k of an [n][m] array starts at ptr + k*n*m; NULL = zero                     */
  const double *x_tan, *xdot_tan, *w_tan, *x_d_tan, *xdot_d_tan, *w_d_tan;   /* [K][n][3]                             */
  const double *Rwb_rot_tan, *Rwb_d_rot_tan;  /* [K][n][3] world-frame left tangent: R <- exp([d]x) R                 */
  const double* feet_tan;        /* [K][n][4][3] body-frame foot position, from `feet` or joint_q                     */
  const double* joint_q_tan;     /* [K][n][12], only with in->joint_q: dp_l = J(q_l) dq_l, added                      */
  double* grf_tan;               /* [K][n][4][3] body frame                                                           */
  double* b_tan;                 /* [K][n][6] optional                                                                */
  int32_t* flags;                /* [n] optional: the bits of qc_sensitivity_io.flags                                 */
} qc_tangent_io;
/* struct_size set, pointers NULL, act_tol = 1e-7, n_dir = 1. */
void qc_default_tangent(qc_tangent_io* io);
/* Asynchronous on `stream`, no host synchronisation (graph-capturable); n == 0 launches nothing and returns QC_OK.
 * QC_ERR_INVALID (message starting with "qc_tangent_batch:", nothing launched) for a null handle, `in` or `io`, a wrong
 * struct_size, an act_tol that is not finite and >= 0, n_dir == 0, neither grf_tan nor b_tan requested, no tangent given at all,
 * joint_q_tan without in->joint_q, a missing grf_body, a missing state array (Rwb, Rwb_d, x, xdot, w, x_d, xdot_d, w_d), neither
 * feet nor joint_q, or n beyond one launch. */
int qc_tangent_batch(qc_handle* h, size_t n, const qc_batch_in* in, const qc_tangent_io* io, void* stream);

/* qc_plant_step_tangent_batch - forward mode of qc_plant_step_batch: K tangents on the inputs of one plant step pushed through it,
 * in one launch.  Given the state BEFORE the step, the forces and the feet the step read (nothing is saved by the forward step; it
 * is recomputed), per direction, in the notation of qc_plant_step_batch (h = Iw w, c = tau - w x h, delta the world-frame left
 * tangent of Rwb, as above; dg_l = grf_tan_l, dp_l = foot_world_tan_l):
 *   df_l  = delta x f_l - Rwb dg_l,   dr_l = dp_l - dx,   da = (sum df_l) / m,   dtau = sum (dr_l x f_l + r_l x df_l)
 *   dh    = delta x h - Iw (delta x w) + Iw dw,   dc = dtau - dw x h - w x dh,   dwdot = Iw^-1 (dc - delta x c) + delta x wdot
 *   dxdot' = dxdot + dt da,   dx' = dx + dt dxdot',   dw' = dw + dt dwdot
 *   delta' = Jl(phi) dt dw' + Exp(phi) delta,  phi = dt w',  Jl = I + B K + C K^2,  K = hat(phi),  B = (1 - cos theta) / theta^2,
 *            C = (theta - sin theta) / theta^3: series in theta^2 below theta^2 = 1, the quotients from it on; at theta = 0 exactly
 *            the smooth limit (Jl = I), as qc_plant_step_adjoint_batch differentiates it
 *   dfeet'_l = Rwb'^T (dp_l - dx' - delta' x d_l),   d_l = foot_world_l - x'.
 * <cotangents of the step's outputs, these tangents> equals <qc_plant_step_adjoint_batch's cotangents, the input tangents>, with the
 * entrywise Rwb_bar paired with [delta]x Rwb and Rwb_next_bar with [delta']x Rwb'.
 *
 * There are no tangents of mass, Ib or dt.  Non-finite inputs propagate as NaN; nothing is clamped.  A (robot, direction) pair
 * reads all its inputs before it writes any output and touches only its own rows, so every output may BE the input tangent of its
 * layout - x_next_tan over x_tan, Rwb_rot_next_tan over Rwb_rot_tan, feet_next_tan over grf_tan or foot_world_tan - and a rollout
 * carries one set of tangent buffers.  The state, force and feet inputs are never written.  All pointers are device pointers.
 *
 * OUT OF SCOPE: tangents of mass, Ib and dt; entrywise rotation tangents.  (The leg plant has its own call,
 * qc_leg_plant_step_tangent_batch, below.) */
typedef struct qc_plant_tangent_io {
  size_t struct_size;            /* = sizeof(qc_plant_tangent_io); checked                                            */
  const double *Rwb;             /* [n][9] the state BEFORE the step                                                  */
  const double *x, *xdot, *w;    /* [n][3]                                                                            */
  const double *grf_body, *foot_world;  /* [n][4][3] as the step read them                                            */
  double dt;                     /* finite, > 0                                                                       */
  size_t n_dir;                  /* K >= 1 directions per launch                                                      */
  /* tangents, direction-major as in qc_tangent_io; NULL = zero, at least one given                                   */
  const double *Rwb_rot_tan, *x_tan, *xdot_tan, *w_tan;   /* [K][n][3]                                                */
  const double *grf_tan;         /* [K][n][4][3] what qc_tangent_batch wrote                                          */
  const double *foot_world_tan;  /* [K][n][4][3]                                                                      */
  /* outputs, each optional, at least one given                                                                       */
  double *Rwb_rot_next_tan, *x_next_tan, *xdot_next_tan, *w_next_tan;  /* [K][n][3]                                   */
  double *feet_next_tan;         /* [K][n][4][3] the tangent of qc_plant_io.feet: the next solve's feet_tan           */
} qc_plant_tangent_io;
/* struct_size set, pointers NULL, dt = 1/300, n_dir = 1. */
void qc_default_plant_tangent(qc_plant_tangent_io* io);
/* Asynchronous on `stream`, no host synchronisation (graph-capturable); n == 0 launches nothing and returns QC_OK.
 * QC_ERR_INVALID (message starting with "qc_plant_step_tangent_batch:", nothing launched) for a null handle or `io`, a wrong
 * struct_size, a dt that is not finite and > 0, n_dir == 0, no tangent given at all, no output requested at all, a missing state,
 * force or feet array, a handle whose mass or Ib qc_plant_step_batch refuses, or n * n_dir beyond one launch. */
int qc_plant_step_tangent_batch(qc_handle* h, size_t n, const qc_plant_tangent_io* io, void* stream);

/* qc_torque_tangent_batch - forward mode of the clamped J^T torque map, the map qc_sensitivity_kin_batch transposes.  Per direction,
 * robot and leg l, with q = joint_q_l, J the leg Jacobian, H_r = d^2 p_r / d q^2, g = grf_body_l, tau_raw = J^T g:
 *   joint_tau_tan_l = m o ( J^T grf_tan_l + (sum_r g_r H_r) joint_q_tan_l )
 * m is qc_sensitivity_kin_batch's mask: m_c = 1 where !(tau_raw_c < tau_min) && !(tau_raw_c > tau_max) (equality passes, a NaN passes
 * and propagates), m = 0 for a swing leg and for a robot with status != 0; the contact mask is resolved as qc_certify_batch
 * resolves it (in->stance, else the phase rule on in->gait_phase with in->gait_duty or the handle's duty, else all stance).  Of `in`
 * only joint_q and the contact inputs are read; nothing is written.  <joint_tau_bar, joint_tau_tan> equals <grf_bar, grf_tan> +
 * <joint_q_bar, joint_q_tan> of qc_sensitivity_kin_batch's torque half.
 *
 * joint_tau_tan may BE grf_tan or joint_q_tan: a (direction, robot, leg) reads all its inputs before it writes and touches only its
 * own row.  Non-finite inputs propagate as NaN where m = 1; nothing is clamped.
 *
 * A swing leg's row is exactly 0: with swing references, qc_swing_torque_tangent_batch (below) called on the same buffer afterwards
 * fills those rows, and joint_tau_tan is the tangent of the tick's complete joint_tau.
 *
 * OUT OF SCOPE: tangents of the kinematic constants and of tau_min / tau_max. */
typedef struct qc_torque_tangent_io {
  size_t struct_size;            /* = sizeof(qc_torque_tangent_io); checked                                           */
  const double* grf_body;        /* [n][4][3] qc_batch_out.grf_body                                                   */
  const int32_t* status;         /* [n] qc_batch_out.status                                                           */
  size_t n_dir;                  /* K >= 1 directions per launch                                                      */
  /* tangents, direction-major as in qc_tangent_io; NULL = zero, at least one given                                   */
  const double* grf_tan;         /* [K][n][4][3] what qc_tangent_batch wrote                                          */
  const double* joint_q_tan;     /* [K][n][12]                                                                        */
  double* joint_tau_tan;         /* [K][n][12] required                                                               */
} qc_torque_tangent_io;
/* struct_size set, pointers NULL, n_dir = 1. */
void qc_default_torque_tangent(qc_torque_tangent_io* io);
/* Asynchronous on `stream`, no host synchronisation (graph-capturable); n == 0 launches nothing and returns QC_OK.
 * QC_ERR_INVALID (message starting with "qc_torque_tangent_batch:", nothing launched) for a null handle, `in` or `io`, a wrong
 * struct_size, n_dir == 0, no output (joint_tau_tan NULL), no tangent given at all, a missing grf_body or status, a missing
 * in->joint_q, or 4 * n * n_dir beyond one launch. */
int qc_torque_tangent_batch(qc_handle* h, size_t n, const qc_batch_in* in, const qc_torque_tangent_io* io, void* stream);

/* qc_swing_torque_tangent_batch - forward mode of the swing legs' PD torques, the map qc_sensitivity_swing_batch transposes: K
 * tangents per launch, chained IN PLACE behind qc_torque_tangent_batch.  Of `in` it reads exactly what qc_sensitivity_swing_batch
 * reads - Rwb, x, joint_q, joint_qdot, swing_pos, swing_vel and the contact inputs resolved by that call's rule (in->stance, else the
 * phase rule on in->gait_phase with in->gait_duty or the handle's duty, else all stance) -; nothing of `in` is written.  Per
 * direction, robot and SWING leg, in the notation of qc_sensitivity_swing_batch (p_b = Rwb^T pos - x (sic), v_b = Rwb^T vel,
 * q_ref = IK(p_b), qd = J(q_ref)^-1 v_b, H_r = d^2 FK_r / dq^2 at q_ref), delta the world-frame left tangent of Rwb:
 *   dp_b   = Rwb^T (dpos - delta x pos) - dx
 *   dv_b   = Rwb^T (dvel - delta x vel)
 *   dq_ref = J(q_ref)^-1 dp_b                      (inside reach the IK inverts the FK)
 *   dqd    = J(q_ref)^-1 (dv_b - B),  B_r = dq_ref^T H_r qd
 *   dtau   = m o ( kp o (dq_ref - dq) + kd o (dqd - dqdot) ) + joint_tau_tan_in
 * m is qc_sensitivity_swing_batch's mask: tau_raw from the forward pass's own function on the same inputs, m_c = 1 where
 * !(tau_raw_c < tau_min) && !(tau_raw_c > tau_max) - the forward tick's mask bit for bit.  The wraps have slope 1; the QP's status
 * plays no part, as in the tick.  A STANCE leg's row is joint_tau_tan_in, or 0 where that is NULL.  qc_torque_tangent_batch writes
 * exact zeros in swing rows, so the two calls in that order on one buffer (joint_tau_tan = joint_tau_tan_in) give the tangent of the
 * tick's complete joint_tau.
 *
 * `flags` follows the adjoint's rules: bit l, swing leg l's reference is out of reach, inside the inner limit, not finite, or at a
 * det J(q_ref) outside the closed-form band.  A flagged leg's row is NaN in every direction, whatever the mask and joint_tau_tan_in;
 * the other legs of that robot are unaffected.  Other non-finite inputs propagate as NaN; nothing else is clamped.
 *
 * <joint_tau_bar, dtau - joint_tau_tan_in> equals <swing_pos_bar, dpos> + <swing_vel_bar, dvel> + <joint_q_bar, dq> +
 * <joint_qdot_bar, dqdot> + <x_bar, dx> + <Rwb_bar, [delta]x Rwb> with the cotangents of qc_sensitivity_swing_batch.
 *
 * joint_tau_tan may BE joint_tau_tan_in or any other [K][n][4][3] input tangent: a (direction, robot, leg) row reads all it needs
 * before it writes and touches only its own row.  All pointers are device pointers.
 *
 * OUT OF SCOPE: tangents of the gains, of tau_min / tau_max and of the kinematic constants; the planner and the gait clock in THIS
 * call (swing_state and gait_dt are refused: qc_swing_reference_tangent_batch, below, gives swing_pos_tan / swing_vel_tan on the
 * references qc_swing_reference_batch returned); commander mode (qc_commander_step_tangent_batch, below, is a call of its own). */
typedef struct qc_swing_tangent_io {
  size_t struct_size;            /* = sizeof(qc_swing_tangent_io); checked                                            */
  size_t n_dir;                  /* K >= 1 directions per launch                                                      */
  /* tangents, direction-major as in qc_tangent_io; NULL = zero, at least one given                                   */
  const double *Rwb_rot_tan, *x_tan;   /* [K][n][3]; Rwb_rot_tan: the world-frame left tangent, Rwb <- exp([d]x) Rwb  */
  const double *swing_pos_tan, *swing_vel_tan, *joint_q_tan, *joint_qdot_tan;  /* [K][n][4][3]                        */
  const double *joint_tau_tan_in;      /* [K][n][4][3] added: what qc_torque_tangent_batch wrote                      */
  double* joint_tau_tan;         /* [K][n][4][3] required unless flags is given                                       */
  int32_t* flags;                /* [n] optional: bit l, swing leg l has no derivative                                */
} qc_swing_tangent_io;
/* struct_size set, pointers NULL, n_dir = 1. */
void qc_default_swing_tangent(qc_swing_tangent_io* io);
/* Asynchronous on `stream`, no host synchronisation (graph-capturable); n == 0 launches nothing and returns QC_OK.
 * QC_ERR_INVALID (message starting with "qc_swing_torque_tangent_batch:", nothing launched) for a null handle, `in` or `io`, a wrong
 * struct_size, n_dir == 0, no tangent given at all, no output (joint_tau_tan and flags both NULL), in->swing_state or in->gait_dt, a
 * missing Rwb, x, joint_q, joint_qdot, swing_pos or swing_vel, or 4 * n * n_dir beyond one launch. */
int qc_swing_torque_tangent_batch(qc_handle* h, size_t n, const qc_batch_in* in, const qc_swing_tangent_io* io, void* stream);

/* qc_leg_plant_step_tangent_batch - forward mode of qc_leg_plant_step_batch: K tangents on the inputs of one step of the legged plant
 * pushed through it, in one launch.  Given the state BEFORE the step (Rwb, x, xdot, w, joint_q, joint_qdot), the torques, the contact
 * inputs (resolved as the step resolves them, cmd_state included), dt and leg_inertia - nothing is saved by the forward step; it is
 * recomputed - per direction, in the notation of qc_leg_plant_step_batch and its adjoint (delta the world-frame left tangent of Rwb,
 * G(g) = sum_r g_r H_r):
 *   stance leg    dp = J dq,  dg = J^-T (dtau - G(g) dq),  df = delta x f - Rwb dg,  dr = delta x r + Rwb dp,  dc = dx + dr
 *   body          qc_plant_step_tangent_batch's block from (df_l, dr_l): da, dtau_body = sum (dr x f + r x df), dh, dc, dwdot, the
 *                 semi-implicit Euler lines, delta' = Jl(phi) dt dw' + Exp(phi) delta (series / quotients / smooth limit as there)
 *   stance leg, after the body has moved
 *                 dp' = Rwb'^T (dc - dx' - delta' x (c - x')),  dqn = J(qn)^-1 dp',  dq' = dqn,  dqd' = (dqn - dq) / dt
 *                 (wrap_PI has slope 1; the IK inverts the FK, so its derivative is the inverse Jacobian at the angles it returned)
 *   swing leg     dqd' = dqd + dt dtau / leg_inertia,  dq' = dq + dt dqd'
 * <cotangents of the step's outputs, these tangents> equals <qc_leg_plant_step_adjoint_batch's cotangents, the input tangents>, with
 * the entrywise Rwb_bar paired with [delta]x Rwb and Rwb_next_bar with [delta']x Rwb'.
 *
 * `flags` carries the adjoint's bits under the adjoint's rules: bit l, J(q_l) of stance leg l is outside the closed-form band;
 * bit 4 + l, leg l is out of reach or J(qn_l) is outside the band.  A robot with any bit set gets NaN in every output row of every
 * direction.  Other non-finite inputs propagate as NaN; nothing is clamped.  A (robot, direction) pair reads all its inputs before
 * it writes and touches only its own rows: each `_next_tan` may BE the input tangent of its layout, and joint_qdot_next_tan may also
 * be joint_tau_tan.  The state and torque inputs are never written.  All pointers are device pointers.
 *
 * OUT OF SCOPE: tangents of mass, Ib, leg_inertia, dt and the kinematic constants; the contact mask is held; entrywise rotation
 * tangents; a tangent of the optional foot_world output of the step. */
typedef struct qc_leg_plant_tangent_io {
  size_t struct_size;               /* = sizeof(qc_leg_plant_tangent_io); checked                                     */
  const double *Rwb, *x, *xdot, *w; /* [n][9], [n][3] x 3: the state BEFORE the step                                  */
  const double *joint_q, *joint_qdot; /* [n][4][3] before the step (joint_qdot's values are not read)                 */
  const double* joint_tau;          /* [n][4][3] the torques the step read                                            */
  const uint8_t* stance;            /* [n][4] optional: the contact inputs of the forward call                        */
  const double* gait_phase;         /* [n][4] optional                                                                */
  const double* gait_duty;          /* [n] optional                                                                   */
  const qc_commander_state* cmd_state; /* [n] optional                                                                */
  double leg_inertia[3];            /* kg m^2 (hip, thigh, calf), finite and > 0: the step's                          */
  double dt;                        /* seconds, finite, > 0: the step's                                               */
  size_t n_dir;                     /* K >= 1 directions per launch                                                   */
  /* tangents, direction-major as in qc_tangent_io; NULL = zero, at least one given                                   */
  const double *Rwb_rot_tan, *x_tan, *xdot_tan, *w_tan;            /* [K][n][3]                                       */
  const double *joint_q_tan, *joint_qdot_tan, *joint_tau_tan;      /* [K][n][12]                                      */
  /* outputs, each optional, at least one given (flags counts)                                                        */
  double *Rwb_rot_next_tan, *x_next_tan, *xdot_next_tan, *w_next_tan;  /* [K][n][3]                                   */
  double *joint_q_next_tan, *joint_qdot_next_tan;                      /* [K][n][12]                                  */
  int32_t* flags;                   /* [n]: bit l singular J(q_l), bit 4 + l out of reach or singular J(qn_l)         */
} qc_leg_plant_tangent_io;
/* struct_size set, pointers NULL, dt = 1/300, n_dir = 1, leg_inertia = 0 (the caller must give the step's). */
void qc_default_leg_plant_tangent(qc_leg_plant_tangent_io* io);
/* Asynchronous on `stream`, no host synchronisation (graph-capturable); n == 0 launches nothing and returns QC_OK.
 * QC_ERR_INVALID (message starting with "qc_leg_plant_step_tangent_batch:", nothing launched) for a null handle or `io`, a wrong
 * struct_size, a dt or a leg_inertia entry that is not finite and > 0, n_dir == 0, no tangent given at all, no output requested at
 * all, a missing Rwb, x, xdot, w, joint_q, joint_qdot or joint_tau, a handle whose mass or Ib qc_plant_step_batch refuses, or
 * n * n_dir beyond one launch. */
int qc_leg_plant_step_tangent_batch(qc_handle* h, size_t n, const qc_leg_plant_tangent_io* io, void* stream);

/* qc_swing_reference_tangent_batch - forward mode of qc_swing_reference_batch (qc_balance.h), the map qc_swing_reference_adjoint_batch
 * transposes: the foothold planner and the sextic swing trajectory, K tangents per launch.  The contract of `in` is the adjoint's,
 * unchanged: nothing is saved by the forward launch; pass the same `in` with gait_phase AS THE FORWARD CALL LEFT IT (gait_dt is
 * refused: no clock is advanced here) and `state_before`, a copy of the qc_swing_state records from BEFORE the forward call.  The
 * plan decision is recomputed from its leg_state / has_traj and the contact mask by the forward kernel's own device functions.  Of
 * `in` it reads Rwb, x, xdot, w, joint_q, gait_phase - required - and the optional stance and gait_duty; `in` is never written.
 *
 * Per direction, robot and leg l, with p = FK(joint_q_l), r = Rwb p, half = t_stance / 2, k = planner_k, lip = sqrt(x_z / 9.81) / 2,
 * hip = planner_hip[l] (the adjoint's symbols), delta the world-frame left tangent of Rwb, dq_l = joint_q_tan_l:
 *   leg replanned:      dr  = delta x r + Rwb J(q_l) dq_l
 *                       dps = dr + dx
 *                       dpf = delta x (Rwb hip) + dx + (half + k + lip) dxdot - k dxdot_d + (0.25 / (9.81 sqrt(x_z / 9.81))) dx_z xdot
 *                             + half (dw x r + w x dr),   dpf_z := 0 (the foothold's z is the constant 0)
 *   leg NOT replanned:  dps = p_start_tan_l,  dpf = p_final_tan_l       (the record passed through)
 *   swing leg with a trajectory after the call, (h, h') the sextic's basis functions and their derivatives at the leg's clamped
 *   trajectory time (the loop the forward kernel and the adjoint share):
 *                       swing_pos_tan_r = (h0 + m h2) dps_r + (h1 + m h2) dpf_r,  swing_vel_tan_r likewise with h'
 *                       m = 1/2 for r = x, y and 0 for z (the centre's z is swing_height)
 *   every other leg:    swing_pos_tan_l = swing_vel_tan_l = 0 exactly
 *   p_start_next_tan_l = dps,  p_final_next_tan_l = dpf                 on the record after the call
 * HELD: the clock, the contact mask and the plan decisions, as in the adjoint.  There is no tangent of the phase, of gait_dt, of the
 * gait's periods, of swing_height, of planner_k or of the kinematic constants.
 *
 * `flags` bit l: leg l is replanned and x_z is not finite and > 0 (the adjoint's rule: the LIP square root has no derivative there).
 * A robot with any bit set gets NaN in every output row of every direction.  Other non-finite inputs propagate; nothing is clamped.
 *
 * <swing_pos_bar, swing_pos_tan> + <swing_vel_bar, swing_vel_tan> + <p_start_next_bar, p_start_next_tan> + <p_final_next_bar,
 * p_final_next_tan> equals <x_bar, dx> + <xdot_bar, dxdot> + <w_bar, dw> + <xdot_d_bar, dxdot_d> + <joint_q_bar, dq> + <p_start_bar,
 * p_start_tan> + <p_final_bar, p_final_tan> + <Rwb_bar, [delta]x Rwb> with the outputs of qc_swing_reference_adjoint_batch (its `_in`
 * arrays NULL): the entrywise Rwb_bar is paired with [delta]x Rwb, as for the other kernels of this header.
 *
 * A (direction, robot) pair reads every input before it writes and touches only its own rows: p_start_next_tan may BE p_start_tan,
 * p_final_next_tan may BE p_final_tan, and swing_pos_tan / swing_vel_tan may be any [K][n][12] input tangent.  A rollout carries the
 * record's two tangents in one pair of buffers.  All pointers are device pointers.  No buffer is kept on the handle.
 *
 * OUT OF SCOPE: tangents of the phase, of gait_dt, of the periods, of swing_height and of planner_k; the commander step and the com
 * reference in THIS call (their forward modes, qc_commander_step_tangent_batch and qc_com_reference_tangent_batch, are below);
 * tangents of the planner's own parameters. */
typedef struct qc_swing_reference_tangent_io {
  size_t struct_size;                         /* = sizeof(qc_swing_reference_tangent_io); checked                      */
  const struct qc_swing_state* state_before;  /* [n] the records before the forward call; required                     */
  size_t n_dir;                               /* K >= 1 directions per launch                                          */
  /* tangents, direction-major as in qc_tangent_io; NULL = zero, at least one given                                   */
  const double *Rwb_rot_tan, *x_tan, *xdot_tan, *w_tan, *xdot_d_tan;  /* [K][n][3]; Rwb_rot_tan: Rwb <- exp([d]x) Rwb  */
  const double* joint_q_tan;                  /* [K][n][12]                                                            */
  const double *p_start_tan, *p_final_tan;    /* [K][n][12] on the record before the call                              */
  /* outputs, each optional, at least one given (flags counts)                                                        */
  double *swing_pos_tan, *swing_vel_tan;      /* [K][n][4][3]                                                          */
  double *p_start_next_tan, *p_final_next_tan;  /* [K][n][12] on the record after the call                             */
  int32_t* flags;                             /* [n]: bit l - replanned leg l has no derivative                        */
} qc_swing_reference_tangent_io;
/* struct_size set, pointers NULL, n_dir = 1. */
void qc_default_swing_reference_tangent(qc_swing_reference_tangent_io* io);
/* Asynchronous on `stream`, no host synchronisation (graph-capturable); n == 0 launches nothing and returns QC_OK.
 * QC_ERR_INVALID (message starting with "qc_swing_reference_tangent_batch:", nothing launched) for a null handle, `in` or `io`, a
 * wrong struct_size, n_dir == 0, no tangent given at all, no output requested at all, a gait_dt, swing_pos or swing_vel in `in`,
 * `feet` without joint_q, a missing state_before, a missing Rwb, x, xdot, w, joint_q or gait_phase, or n * n_dir beyond one launch. */
int qc_swing_reference_tangent_batch(qc_handle* h, size_t n, const qc_batch_in* in, const qc_swing_reference_tangent_io* io, void* stream);

/* qc_commander_step_tangent_batch - forward mode of qc_commander_step_batch (qc_balance.h), the map qc_commander_step_adjoint_batch
 * transposes: from K tangents on the twist command, the held command, the pose and the record's desired state to the tangents of the
 * desired state the QP and the planner are fed.  The contract is the adjoint's: nothing is saved by the forward launch; pass the same
 * Rwb and x (`in`), twist, fresh and the three scalars (`cmd`; cmd->state is not read) and `state_before`, a copy of the records from
 * BEFORE the forward call.  fresh / standing / running / pending / applied are recomputed as the forward kernel decides them and HELD.
 *
 * Per direction, in the symbols of qc_commander_step_adjoint_batch (v = vb[0:3], om = vb[3:6], d = cmd_dt om, Rb = Exp(d),
 * t = cmd_dt Rb v, Y = Rz(yaw), (cy, sy) = (R00, R10) / h, u = v - x x om), delta = Rwb_rot_tan, dx = x_tan,
 * dvb = fresh ? twist_tan : Vb_tan = (dv, dom):
 *   always        Vb_next_tan = dvb
 *   NOT applied   the four desired-state outputs are the four `_prev_` tangents, bit for bit; nothing else reaches them
 *   applied       beta = Jl(d) cmd_dt dom                     (the left tangent of Rb)
 *                 dt   = beta x t + cmd_dt Rb dv
 *                 dpsi = (cy (delta_2 R00 - delta_0 R20) - sy (delta_1 R20 - delta_2 R10)) / h
 *                 Rwb_d_rot_tan = dpsi e_z + Y beta
 *                 x_d_tan = (dx_0 + g_0, dx_1 + g_1, 0),  g = dpsi e_z x (Y t) + Y dt      (the height is a constant)
 *                 xdot_d_tan = Rwb^T (du - delta x u),  du = dv - dx x om - x x dom
 *                 w_d_tan = Rwb^T (dom - delta x om)
 * SMALL ANGLE, |d| < 1e-12, where the forward pass takes Rb = I: the SMOOTH function is differentiated, as the adjoint does - a
 * yaw-rate tangent at zero rate is not silently zero.  Jl = I + B K + C K^2 by qc_plant_step_tangent_batch's coefficients: the series
 * below |d|^2 = 1, the quotients from it on, Jl = I at |d| = 0.
 *
 * Rwb_d_rot_tan, x_d_tan, xdot_d_tan, w_d_tan are exactly what qc_tangent_batch and qc_swing_reference_tangent_batch take under those
 * names (Rwb_d_rot_tan: the world-frame left tangent of Rwb_d).
 *
 * `flags` bit 0 is the adjoint's rule: a command is applied at the gimbal-lock branch (h == 0 or not finite below 1e300).  Every
 * output row of that robot, in every direction, is NaN.  Other non-finite inputs propagate; nothing is clamped.  There are no tangents
 * of stand_height, stand_tol or cmd_dt; the flags and latches are held.
 *
 * <G, [Rwb_d_rot_tan]x Rwb_d> + <a, x_d_tan> + <b, xdot_d_tan> + <c, w_d_tan> + <Vb_next_bar, Vb_next_tan> equals <twist_bar, twist_tan>
 * + <Vb_bar, Vb_tan> + <Rwb_bar, [delta]x Rwb> + <x_bar, dx> + <Rwb_d_prev_bar, [Rwb_d_rot_prev_tan]x Rwb_d_prev> + <x_d_prev_bar,
 * x_d_prev_tan> + <xdot_d_prev_bar, xdot_d_prev_tan> + <w_d_prev_bar, w_d_prev_tan> with the outputs of
 * qc_commander_step_adjoint_batch (its `_in` arrays NULL; G = Rwb_d_bar, a = x_d_bar, b = xdot_d_bar, c = w_d_bar).
 *
 * A (direction, robot) pair reads every input before it writes and touches only its own rows: the four desired-state outputs may BE
 * the four `_prev_` inputs and Vb_next_tan may BE Vb_tan - a rollout carries them in one set of buffers.  All pointers are device
 * pointers.  No buffer is kept on the handle.
 *
 * OUT OF SCOPE: tangents of stand_height, stand_tol and cmd_dt; entrywise rotation tangents. */
typedef struct qc_commander_step_tangent_io {
  size_t struct_size;                             /* = sizeof(qc_commander_step_tangent_io); checked                   */
  const struct qc_commander_state* state_before;  /* [n] the records before the forward call; required                 */
  size_t n_dir;                                   /* K >= 1 directions per launch                                      */
  /* tangents, direction-major as in qc_tangent_io; NULL = zero, at least one given                                   */
  const double *twist_tan, *Vb_tan;               /* [K][n][6]; twist_tan only with cmd->twist                         */
  const double *Rwb_rot_tan, *x_tan;              /* [K][n][3]; Rwb_rot_tan: Rwb <- exp([d]x) Rwb                      */
  const double *Rwb_d_rot_prev_tan, *x_d_prev_tan, *xdot_d_prev_tan, *w_d_prev_tan;  /* [K][n][3] on the record before */
  /* outputs, each optional, at least one given (flags counts)                                                        */
  double *Rwb_d_rot_tan, *x_d_tan, *xdot_d_tan, *w_d_tan;  /* [K][n][3]                                                */
  double* Vb_next_tan;                            /* [K][n][6] on the held command after the call                      */
  int32_t* flags;                                 /* [n]: bit 0 - applied at gimbal lock, no derivative                */
} qc_commander_step_tangent_io;
/* struct_size set, pointers NULL, n_dir = 1. */
void qc_default_commander_step_tangent(qc_commander_step_tangent_io* io);
/* Asynchronous on `stream`, no host synchronisation (graph-capturable); n == 0 launches nothing and returns QC_OK.
 * QC_ERR_INVALID (message starting with "qc_commander_step_tangent_batch:", nothing launched) for a null handle, `in`, `cmd` or `io`,
 * a wrong struct_size of either record, n_dir == 0, no tangent given at all, no output requested at all, twist_tan without
 * cmd->twist, `fresh` without `twist`, a stand_height, stand_tol (>= 0) or cmd_dt that is not finite, a missing state_before, Rwb or
 * x, or n * n_dir beyond one launch. */
int qc_commander_step_tangent_batch(qc_handle* h, size_t n, const qc_batch_in* in, const qc_command_in* cmd,
                                    const qc_commander_step_tangent_io* io, void* stream);

/* qc_com_reference_tangent_batch - forward mode of qc_com_reference_batch (qc_balance.h), the map qc_com_reference_adjoint_batch
 * transposes: the desired COM from the virtual support polygon, K tangents per launch.  It takes the same `in`, schedule,
 * schedule_shared, mode and gain; nothing is saved by the forward launch.  The contact mask is HELD: a phase exactly on the stance /
 * swing boundary gets the branch the forward pass took.
 *
 * Per direction, robot and leg l, with p_l the body-frame foot (`feet`, or the FK of joint_q), r_l = Rwb p_l, delta = Rwb_rot_tan,
 * dx = x_tan, dphi = phase_tan, dsigma = schedule_tan, and a_i, d_i, e_i = exp(-a_i^2) / sqrt(pi), sgn those of
 * qc_support_polygon_adjoint_batch:
 *   dp_l = feet_tan_l + J(q_l) joint_q_tan_l                                         (as in qc_tangent_batch)
 *   dP_l = (delta x r_l + Rwb dp_l + dx) in x and y
 *   dw_l = sgn (e1 / d1 - e2 / d2) dphi_l - sum_i e_i a_i sqrt(2) / d_i dsigma_i     over the two widths the leg's branch reads
 *   dzm = w dP + (1 - w) dP_m + (P - P_m) dw, dzp likewise;  with v = N / D: dv = (dN - v dD) / D, in the forward pass's own
 *   summation order;  com_xy_tan = (((dv_FL + dv_FR) + dv_RL) + dv_RR) / 4
 *   QC_COM_REPLACE   x_d_out_tan = (com_xy_tan, x_d_in_tan.z)
 *   QC_COM_OFFSET    x_d_out_tan = x_d_in_tan + gain (com_xy_tan - (((dP_FL + dP_FR) + dP_RL) + dP_RR) / 4, 0)
 * `gain` has no tangent.  With schedule_shared, schedule_tan is ONE [4][4] block per direction, [K][4][4].
 *
 * `flags` bit l: the forward rule, the reference's 0/0 at leg l's point.  A flagged robot gets NaN in every output row of every
 * direction.  Other non-finite inputs propagate; nothing is clamped.
 *
 * <x_d_out_bar, x_d_out_tan> equals <x_d_in_bar, x_d_in_tan> + <feet_bar, dp> + <Rwb_bar, [delta]x Rwb> + <x_bar, dx> + <phase_bar,
 * dphi> + <schedule_bar rows, dsigma> with the outputs of qc_com_reference_adjoint_batch (its `_in` arrays NULL); with a shared
 * schedule_tan the last term is <schedule_bar_sum, dsigma> over the batch.  com_xy_tan in replace mode is the tangent of
 * qc_support_polygon_batch's world-mode com_xy: there is no separate call for it.
 *
 * A (direction, robot) pair reads every input before it writes and touches only its own rows: x_d_out_tan may BE x_d_in_tan.  All
 * pointers are device pointers.  No buffer is kept on the handle.
 *
 * OUT OF SCOPE: tangents of gain and of the phase through the clock; the body-frame polygon. */
typedef struct qc_com_reference_tangent_io {
  size_t struct_size;            /* = sizeof(qc_com_reference_tangent_io); checked                                    */
  const double* schedule;        /* as the forward call's                                                             */
  int32_t schedule_shared;
  int32_t mode;
  double gain;
  size_t n_dir;                  /* K >= 1 directions per launch                                                      */
  /* tangents, direction-major as in qc_tangent_io; NULL = zero, at least one given                                   */
  const double* x_d_in_tan;      /* [K][n][3]                                                                         */
  const double* feet_tan;        /* [K][n][4][3] body frame                                                           */
  const double* joint_q_tan;     /* [K][n][12], only with in->joint_q                                                 */
  const double *Rwb_rot_tan, *x_tan;  /* [K][n][3]                                                                    */
  const double* phase_tan;       /* [K][n][4]                                                                         */
  const double* schedule_tan;    /* [K][n][4][4], or [K][4][4] with schedule_shared                                   */
  /* outputs, each optional, at least one given (flags counts)                                                        */
  double* x_d_out_tan;           /* [K][n][3]; may be x_d_in_tan                                                      */
  double* com_xy_tan;            /* [K][n][2] the polygon's own tangent                                               */
  int32_t* flags;                /* [n]: bit l - leg l's point is 0/0, no derivative                                  */
} qc_com_reference_tangent_io;
/* struct_size set, mode = QC_COM_REPLACE, gain = 1, n_dir = 1, the rest zero. */
void qc_default_com_reference_tangent(qc_com_reference_tangent_io* io);
/* Asynchronous on `stream`, no host synchronisation (graph-capturable); n == 0 launches nothing and returns QC_OK.
 * QC_ERR_INVALID (message starting with "qc_com_reference_tangent_batch:", nothing launched) for a null handle, `in` or `io`, a wrong
 * struct_size, a gait_dt, swing_state, swing_pos or swing_vel in `in`, an unknown mode, a gain that is not finite, n_dir == 0, no
 * tangent given at all, no output requested at all, joint_q_tan without in->joint_q, a missing schedule, gait_phase, feet / joint_q,
 * Rwb or x, or n * n_dir beyond one launch. */
int qc_com_reference_tangent_batch(qc_handle* h, size_t n, const qc_batch_in* in, const qc_com_reference_tangent_io* io, void* stream);

/* qc_param_tangent_batch - forward mode of the balance QP in the handle's own PARAMETERS, the map qc_sensitivity_param_batch
 * (qc_balance.h) transposes: K directions in the QC_PARAM_COUNT = 211 doubles of qc_params - mu, mass, fzmin, fzmax, Ib[9], S[36],
 * W[144], kff[6], kp_p[3], kd_p[3], kp_w[3], kd_w[3], matrices entrywise and row-major - pushed through the QP on its active face.
 * The handle holds ONE parameter set for the batch, so param_tan is SHARED by the batch: [K][211], not [K][n][211].  The call takes
 * the SAME qc_batch_in the solve read and the forces; the face is exactly qc_tangent_batch's (qc_certify_batch's codes at act_tol; a
 * code 3 on any axis of a foot pins that foot and sets bit 0 of `flags`), `in` is never written.
 *
 * In the notation of qc_sensitivity_param_batch - f the world forces, u = A f - b, v = S u, g = 2 (A^T v + W f),
 * H = 2 (A^T S A + W), sx, sy in {-1, 0, +1} from the x / y codes 1 / 2 / 0 of a foot - per direction:
 *   db     the forward derivative of the PD law in mass, kff, kp_p, kd_p, kp_w, kd_w and Ib, line by line as the library evaluates
 *          it: db_lin = dmass (a - (0, 0, 9.81)) + mass da with da = dkp_p o (x_d - x) + dkd_p o (xdot_d - xdot) + (dkff0 xdot_d0,
 *          dkff1 xdot_d1, dkff2 mass 9.81 + kff2 dmass 9.81) (mass enters three times); dal = dkp_w o e + dkd_w o (w_d - w) +
 *          (dkff3 w_d0, dkff4 w_d1 + dkff5 w_d2, 0) (kff[5] acts on the second component, as the library has it);
 *          db_ang = Iw dal + dIw al + w_d x (dIw w_d) with dIw = Rwb dIb Rwb^T
 *   dg     = 2 (A^T dS u + dW f - A^T S db) at fixed f; dS and dW are taken entrywise AS GIVEN, not symmetrised - the caller owns
 *          that, as with S_bar / W_bar
 *   df0_l  the motion of foot l at fixed free coordinates: (sx, sy, 0) f_lz dmu with fz free; (sx (dmu f_lz + mu dfzmin),
 *          sy (dmu f_lz + mu dfzmin), dfzmin) at a z code 1 (f_lz is fzmin there, to act_tol; the adjoint reads f_lz and so does
 *          this); the same with fzmax at a z code 2; nothing for a swing foot or a foot with a code 3
 *   dZ^T g on the z column of each foot with fz free: dmu (sx g_lx + sy g_ly)
 *   (Z^T H Z) dy = -Z^T (H df0 + dg) - dZ^T g             (factorised once per robot, substituted K times)
 *   df = df0 + Z dy,   grf_tan_l = -Rwb^T df_l (+ grf_tan_in),   b_tan = db (+ b_tan_in).
 * <grf_bar, grf_tan_k - grf_tan_in_k> per robot equals <param_bar_rows' row, param_tan_k> with what qc_sensitivity_param_batch writes
 * for that grf_bar.  With unit seeds the K outputs are K columns of d grf_body / d theta.
 *
 * This is the derivative of the CONTROLLER's use of mass and Ib (the wrench law), as the cotangent is; a plant that integrates the
 * same body is another function of them.
 *
 * A pivot that is not positive and finite sets bit 1 of `flags`, and every grf_tan and b_tan of that robot is NaN in all K
 * directions - a grf_tan_in does not rescue it.  A failed robot (all-zero forces), and a robot with no stance foot whose forces are
 * zero, gets grf_tan = grf_tan_in + 0: grf_tan_in's numbers exactly (of its bits only the sign of a -0.0 may change), or exact
 * zeros without one; b_tan is still db (+ b_tan_in).  Non-finite inputs propagate; nothing is clamped.
 *
 * grf_tan_in may BE grf_tan and b_tan_in may BE b_tan: a (direction, robot) pair reads its rows before it writes them and touches
 * only its own.  qc_tangent_batch followed by this call with grf_tan_in = grf_tan on its buffer gives the tangent in the state and
 * the parameters together: the sum of the two calls run apart, bit for bit (one IEEE addition of the two results).  param_tan must
 * not overlap an output.  All pointers are device pointers.  No buffer is kept on the handle.
 *
 * OUT OF SCOPE: per-robot parameter directions; tangents of the kinematic model, of tau_min / tau_max, of the joint gains and of the
 * plant's use of mass and Ib (qc_plant_step_tangent_batch and qc_leg_plant_step_tangent_batch hold them; the reverse mode in
 * the plant's own mass and Ib is qc_plant_step_model_adjoint_batch, include/qc_plant_model.h); symmetrised dS / dW;
 * fusing this launch with qc_tangent_batch - it repeats that call's classification and factorisation (profiles/param_tangent.md
 * has what that costs). */
typedef struct qc_param_tangent_io {
  size_t struct_size;            /* = sizeof(qc_param_tangent_io); checked                                            */
  const double* grf_body;        /* [n][4][3] qc_batch_out.grf_body                                                   */
  double act_tol;                /* as qc_sensitivity_io.act_tol: finite, >= 0                                        */
  size_t n_dir;                  /* K >= 1 directions per launch                                                      */
  const double* param_tan;       /* [K][QC_PARAM_COUNT], SHARED by the batch, qc_params' order, matrices entrywise     */
  const double* grf_tan_in;      /* [K][n][4][3] optional: added; may BE grf_tan                                      */
  const double* b_tan_in;        /* [K][n][6] optional: added; may BE b_tan                                           */
  double* grf_tan;               /* [K][n][4][3] body frame                                                           */
  double* b_tan;                 /* [K][n][6] optional                                                                */
  int32_t* flags;                /* [n] optional: the bits of qc_sensitivity_io.flags                                 */
} qc_param_tangent_io;
/* struct_size set, pointers NULL, act_tol = 1e-7, n_dir = 1. */
void qc_default_param_tangent(qc_param_tangent_io* io);
/* Asynchronous on `stream`, no host synchronisation (graph-capturable); n == 0 launches nothing and returns QC_OK.
 * QC_ERR_INVALID (message starting with "qc_param_tangent_batch:", nothing launched) for a null handle, `in` or `io`, a wrong
 * struct_size, an act_tol that is not finite and >= 0, n_dir == 0, a missing param_tan, neither grf_tan nor b_tan requested,
 * grf_tan_in without grf_tan, b_tan_in without b_tan, a missing grf_body, a missing state array (Rwb, Rwb_d, x, xdot, w, x_d, xdot_d,
 * w_d), neither feet nor joint_q, or n beyond one launch. */
int qc_param_tangent_batch(qc_handle* h, size_t n, const qc_batch_in* in, const qc_param_tangent_io* io, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* QC_TANGENT_H */
