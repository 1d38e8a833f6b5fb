/* qc_tangent.h - forward mode of the balance QP: qc_tangent_batch pushes K tangents on the inputs of a solved batch through the
 * QP on its active face and returns the tangents of the forces.  A header beside qc_balance.h: the two functions live in the same
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
 * the handle's parameters (mu, fzmin, fzmax, the weights, the gains, mass, Ib, the kinematic model); tangents through the J^T
 * torque map, the leg plant and the swing pipeline; weak activity (a row whose multiplier is about 0 is on the face like any other);
 * commander mode (the desired state must be in `in`); a jvp on the torch.autograd.Functions of the Python package.
 *
 * The rigid-body plant step has its forward mode below, qc_plant_step_tangent_batch: with it the two calls chain, step after step,
 * into the tangent of a closed-loop rollout. */
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
 * OUT OF SCOPE: the leg plant (qc_leg_plant_step_batch); tangents of mass, Ib and dt; entrywise rotation tangents. */
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

#ifdef __cplusplus
}
#endif
#endif /* QC_TANGENT_H */
