/* qc_plant_model.h - a plant of its own: the two plant steps of qc_balance.h with a PER-ROBOT body (mass, inertia) and an external
 * wrench, and the reverse pass of the rigid-body one with the cotangents of all three.  A header beside qc_balance.h, as
 * qc_tangent.h is: its functions live in the same libqc_balance.so, QC_ABI_VERSION and the records of qc_balance.h are untouched.
 *
 * qc_plant_step_batch and qc_leg_plant_step_batch integrate the handle's mass and Ib - the numbers the QP itself assumes - and apply
 * no force the controller did not ask for.  The calls below are EXACTLY those steps, with their records and their contracts (state
 * updated in place, every input of a robot read before any of its outputs is written, optional feet / foot_world / flags,
 * asynchronous launch without host synchronisation), and three differences:
 *   wrench  fs and tau start from (F, M) = wrench_world[i] - a force at the centre of mass, then a moment about it, world frame, held
 *           over the step - instead of from +0.0; the per-leg terms are added in the base kernel's order, so a wrench array of +0.0
 *           alone gives the base kernel's result bit for bit.
 *   mass    the robot's own m goes into a = fs / m - g e_z.
 *   Ib      the robot's own nine entries go into Ib (Rwb^T w), and their general 3x3 inverse - the adjugate over the determinant, from
 *           all nine entries as given; no symmetry is assumed by the arithmetic, so an entrywise derivative is well defined - into
 *           Ib^-1 Rwb^T (...).
 * `flags`, if given, receives per robot: bit 0 - mass is not finite or <= 0; bit 1 - Ib is refused: an entry is not finite, or
 * Sylvester's three leading minors (Ib[0], Ib[0] Ib[4] - Ib[1] Ib[3], the determinant), computed from the entries as given, are not
 * all positive, or |Ib[ab] - Ib[ba]| exceeds 1e-12 max|Ib|.  Every state output of a flagged robot's step is NaN (Rwb, x, xdot, w,
 * and feet, or joint_q and joint_qdot), with or without the array; its neighbours are untouched.  The leg plant's own `flags` word
 * and its foot_world keep their meaning.
 *
 * OUT OF SCOPE: the leg plant's adjoint with a model; forward-mode (tangent) twins; a model inside qc_tick_batch or the solve (the
 * QP keeps the handle's mass and Ib: the mismatch is the point); per-robot g, dt, leg_inertia; a wrench applied at a body point
 * (callers shift the moment themselves: M += (p - x) x F); a batch-summed mass_bar / Ib_bar (the caller sums the rows); any contact
 * model. */
#ifndef QC_PLANT_MODEL_H
#define QC_PLANT_MODEL_H

#include "qc_balance.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct qc_plant_model {
  size_t struct_size;         /* = sizeof(qc_plant_model); checked                                                              */
  const double* mass;         /* [n]    optional (NULL: the handle's mass)                                                      */
  const double* Ib;           /* [n][9] optional, row-major (NULL: the handle's Ib and the inverse the handle holds)            */
  const double* wrench_world; /* [n][6] optional: force at the centre of mass, then moment about it, world frame, held over the step */
  int32_t* flags;             /* [n]    optional OUT: bit 0 mass not finite or <= 0; bit 1 Ib refused (above)                   */
} qc_plant_model;
/* struct_size set, pointers NULL. */
void qc_default_plant_model(qc_plant_model* model);

/* qc_plant_step_batch on the model's body.  QC_ERR_INVALID (message starting with "qc_plant_step_model_batch:", nothing launched)
 * for everything qc_plant_step_batch refuses, a NULL `model`, a wrong model->struct_size, and a model whose mass, Ib and
 * wrench_world are all NULL (call qc_plant_step_batch; n == 0 reads no array and launches nothing, with such a model too).  A handle whose mass or Ib the base call refuses is accepted when the model
 * supplies that quantity. */
int qc_plant_step_model_batch(qc_handle* h, size_t n, const qc_plant_io* io, const qc_plant_model* model, void* stream);
/* qc_leg_plant_step_batch on the model's body, in the same way (messages start with "qc_leg_plant_step_model_batch:"). */
int qc_leg_plant_step_model_batch(qc_handle* h, size_t n, const qc_leg_plant_io* io, const qc_plant_model* model, void* stream);

/* The reverse pass of qc_plant_step_model_batch: qc_plant_step_adjoint_batch on the model's step - the existing six outputs through
 * the existing record - and the cotangents of the model, in the names of the step (wb = Rwb^T w, Iwb = Ib wb, nb = Rwb^T tau,
 * Inb = Ib^-1 nb, a = fs / m - g e_z):
 *   wrench_bar = (fs_bar, tau_bar)                        the two cotangents the pass forms on the way to grf_bar
 *   mass_bar   = -<fs, a_bar> / m^2
 *   Ib_bar     = Iwb_bar wb^T - (Ib^-T Inb_bar) Inb^T     ENTRYWISE and unsymmetrised, as qc_sensitivity_param_batch's rows for Ib
 * mass_bar and Ib_bar are also produced when the model takes that quantity from the handle: they are then per-robot rows of the
 * handle's cotangent, and the caller sums them.  Outputs are written, not accumulated; an output may be the same array as an input
 * cotangent of its layout (wrench_bar has no such twin).  A flagged robot (`flags`: the forward call's bits, recomputed) gets NaN in
 * every output of its row, the existing record's included.  Nothing is saved by the forward call. */
typedef struct qc_plant_model_bar {
  size_t struct_size; /* = sizeof(qc_plant_model_bar); checked                          */
  double* wrench_bar; /* [n][6] optional                                                */
  double* mass_bar;   /* [n]    optional                                                */
  double* Ib_bar;     /* [n][9] optional, ENTRYWISE, unsymmetrised                      */
  int32_t* flags;     /* [n]    optional: the forward call's bits, recomputed           */
} qc_plant_model_bar;
/* struct_size set, pointers NULL. */
void qc_default_plant_model_bar(qc_plant_model_bar* bar);
/* QC_ERR_INVALID (message starting with "qc_plant_step_model_adjoint_batch:", nothing launched) for everything
 * qc_plant_step_adjoint_batch refuses - except that the existing record may request no output if `bar` requests one (wrench_bar,
 * mass_bar or Ib_bar), and `bar` may be NULL if the existing record requests one -, for a NULL `model`, a wrong struct_size of
 * `model` or `bar`, and a model whose mass, Ib and wrench_world are all NULL.  A handle whose mass or Ib the base call refuses is
 * accepted when the model supplies that quantity. */
int qc_plant_step_model_adjoint_batch(qc_handle* h, size_t n, const qc_plant_adjoint_io* io, const qc_plant_model* model,
                                      const qc_plant_model_bar* bar, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* QC_PLANT_MODEL_H */
