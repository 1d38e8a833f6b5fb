// The device-free host logic of the parameter-cotangent entry point (quadruped_control_amd/csrc/qc_host.hpp):
// check_sensitivity_param_args through every refusal of qc_sensitivity_param_batch, the launch grid, and the table that makes each
// of the 211 entries a product of two slots of a lane's record (csrc/qc_sensitivity_params.hpp).  Host compiler only - links neither
// HIP nor the library; built with the address and undefined-behaviour sanitizers (__graft_entry__.build_host_test) and run by
// tests/test_sensitivity_params_cpu.py.  Prints the failing case and exits 1 on the first violated check.
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <string>

#include "host_check.hpp"

using namespace qc;

static double buf[4];
static uint8_t bytes[4];

static qc_batch_in valid_in() {
  qc_batch_in in{};
  in.Rwb = in.Rwb_d = in.x = in.xdot = in.w = in.x_d = in.xdot_d = in.w_d = in.feet = buf;
  return in;
}
static qc_sensitivity_param_io valid_io() {
  qc_sensitivity_param_io io{};
  io.struct_size = sizeof(qc_sensitivity_param_io);
  io.grf_body = io.grf_bar = io.adjoint = buf;
  io.act_tol = 1e-7;
  io.param_bar = buf;
  return io;
}

static void arguments() {
  const qc_handle* const h = reinterpret_cast<const qc_handle*>(buf);  // only compared with null
  const qc_batch_in in = valid_in();
  const qc_sensitivity_param_io io = valid_io();
  CHECK(check_sensitivity_param_args(h, 1, &in, &io) == QC_OK, "the smallest valid call (the sum alone)");
  {
    qc_batch_in b = in;
    b.feet = nullptr; b.joint_q = buf; b.stance = bytes; b.gait_phase = buf; b.gait_duty = buf;
    b.gait_dt = buf; b.swing_pos = b.swing_vel = b.joint_qdot = buf;  // ignored, not refused
    qc_sensitivity_param_io c = io;
    c.param_bar_rows = buf;
    c.act_tol = 0.0;
    CHECK(check_sensitivity_param_args(h, 65537, &b, &c) == QC_OK, "joint_q, every optional input and both outputs");
  }
  const char* const null_arg = "qc_sensitivity_param_batch: null argument";
  CHECK_FAILS(check_sensitivity_param_args(nullptr, 1, &in, &io), null_arg, "no handle");
  CHECK_FAILS(check_sensitivity_param_args(h, 1, nullptr, &io), null_arg, "no in");
  CHECK_FAILS(check_sensitivity_param_args(h, 1, &in, nullptr), null_arg, "no io");
  CHECK_FAILS(check_sensitivity_param_args(nullptr, 0, &in, &io), null_arg, "no handle, n = 0");
  for (const size_t sz : {(size_t)0, sizeof(qc_sensitivity_param_io) - 8, sizeof(qc_sensitivity_param_io) + 8, sizeof(qc_sensitivity_rot_io)}) {
    qc_sensitivity_param_io c = io;
    c.struct_size = sz;
    char text[320];
    std::snprintf(text, sizeof text,
                  "qc_sensitivity_param_batch: qc_sensitivity_param_io.struct_size is %zu, this library's qc_sensitivity_param_io has %zu B (qc_default_sensitivity_param sets it)",
                  sz, sizeof(qc_sensitivity_param_io));
    CHECK_FAILS(check_sensitivity_param_args(h, 1, &in, &c), text, "struct_size %zu", sz);
    CHECK_FAILS(check_sensitivity_param_args(h, 0, &in, &c), text, "struct_size %zu, n = 0", sz);
  }
  const char* const tol = "qc_sensitivity_param_batch: act_tol must be finite and >= 0";
  for (const double t : {-1e-300, -1.0, (double)INFINITY, -(double)INFINITY, (double)NAN}) {
    qc_sensitivity_param_io c = io;
    c.act_tol = t;
    CHECK_FAILS(check_sensitivity_param_args(h, 1, &in, &c), tol, "act_tol %g", t);
    CHECK_FAILS(check_sensitivity_param_args(h, 0, &in, &c), tol, "act_tol %g, n = 0", t);
    c.param_bar = nullptr;  // (the tolerance is judged before the outputs)
    CHECK_FAILS(check_sensitivity_param_args(h, 1, &in, &c), tol, "act_tol %g and no output", t);
  }
  {
    qc_sensitivity_param_io c = io;
    c.param_bar = nullptr;
    const char* const none = "qc_sensitivity_param_batch: no output requested (param_bar_rows and param_bar are both NULL)";
    CHECK_FAILS(check_sensitivity_param_args(h, 1, &in, &c), none, "no output");
    CHECK_FAILS(check_sensitivity_param_args(h, 0, &in, &c), none, "no output, n = 0");
    c.param_bar_rows = buf;
    CHECK(check_sensitivity_param_args(h, 1, &in, &c) == QC_OK, "the rows alone");
  }
  const char* const inputs = "qc_sensitivity_param_batch: grf_body, grf_bar and adjoint are required";
  const double* qc_sensitivity_param_io::* const ins[] = {&qc_sensitivity_param_io::grf_body, &qc_sensitivity_param_io::grf_bar, &qc_sensitivity_param_io::adjoint};
  for (size_t m = 0; m < sizeof(ins) / sizeof(ins[0]); m++) {
    qc_sensitivity_param_io c = io;
    c.*ins[m] = nullptr;
    CHECK_FAILS(check_sensitivity_param_args(h, 1, &in, &c), inputs, "input %zu missing", m);
    CHECK(check_sensitivity_param_args(h, 0, &in, &c) == QC_OK, "input %zu missing, n = 0 asks for no array", m);
  }
  const char* const state =
      "qc_sensitivity_param_batch: the state arrays Rwb, Rwb_d, x, xdot, w, x_d, xdot_d and w_d are required (commander mode is out of scope)";
  const double* qc_batch_in::* const members[] = {&qc_batch_in::Rwb, &qc_batch_in::Rwb_d, &qc_batch_in::x, &qc_batch_in::xdot,
                                                  &qc_batch_in::w, &qc_batch_in::x_d, &qc_batch_in::xdot_d, &qc_batch_in::w_d};
  for (size_t m = 0; m < sizeof(members) / sizeof(members[0]); m++) {
    qc_batch_in b = in;
    b.*members[m] = nullptr;
    CHECK_FAILS(check_sensitivity_param_args(h, 1, &b, &io), state, "state array %zu missing", m);
    CHECK(check_sensitivity_param_args(h, 0, &b, &io) == QC_OK, "state array %zu missing, n = 0", m);
  }
  {
    qc_batch_in b = in;
    b.Rwb_d = b.x_d = b.xdot_d = b.w_d = nullptr;
    b.feet = nullptr; b.joint_q = buf;
    CHECK_FAILS(check_sensitivity_param_args(h, 1, &b, &io), state, "a commander-mode batch");
  }
  {
    qc_batch_in b = in;
    b.feet = nullptr;
    CHECK_FAILS(check_sensitivity_param_args(h, 1, &b, &io), "qc_sensitivity_param_batch: feet or joint_q is required", "neither feet nor joint_q");
    b.joint_q = buf;
    CHECK(check_sensitivity_param_args(h, 1, &b, &io) == QC_OK, "joint_q in place of feet");
  }
  const size_t most = (size_t)0xFFFFFF * SENSITIVITY_PARAM_BLOCK;
  CHECK(check_sensitivity_param_args(h, most, &in, &io) == QC_OK, "the largest batch of one launch");
  CHECK_FAILS(check_sensitivity_param_args(h, most + 1, &in, &io), "qc_sensitivity_param_batch: n is beyond one launch", "one robot more");
  CHECK(sizeof(qc_sensitivity_param_io) == 7 * 8, "the io record: struct_size, three inputs, act_tol and two outputs");
  CHECK(sizeof(qc_sensitivity_io) == 14 * 8 && sizeof(qc_sensitivity_rot_io) == 9 * 8, "the two earlier io records keep their sizes");
}

static void grid() {
  CHECK(sensitivity_param_blocks(1) == 1 && sensitivity_param_blocks(64) == 1 && sensitivity_param_blocks(65) == 2, "one wave per 64 robots");
  CHECK(sensitivity_param_blocks(1025) == 17, "1025 robots: one partial more than the finisher has waves");
  CHECK(sensitivity_param_blocks(65536) == 1024 && sensitivity_param_blocks(65537) == 1024 && sensitivity_param_blocks((size_t)1 << 30) == 1024,
        "capped at the handle's partial buffer");
  CHECK(SENSITIVITY_PARAM_MAX_BLOCKS <= SENSITIVITY_PARAM_SUM_BLOCK && SENSITIVITY_PARAM_SUM_BLOCK % 64 == 0 && PARAM_COUNT <= SENSITIVITY_PARAM_SUM_BLOCK,
        "the finisher has a thread per entry");
  CHECK(sensitivity_blocks(65537) == 1025 && certify_blocks(65537) == 1025, "the other per-robot grids keep their cap");
}

// the layout of a cotangent is the order of qc_params' doubles; each entry is one product of two record slots
static void layout() {
  CHECK(QC_PARAM_COUNT == 211 && PARAM_COUNT == QC_PARAM_COUNT && offsetof(qc_params, max_iter) == 8 * QC_PARAM_COUNT, "211 doubles, then max_iter");
  CHECK(offsetof(qc_params, Ib) == 8 * 4 && offsetof(qc_params, S) == 8 * 13 && offsetof(qc_params, W) == 8 * 49 && offsetof(qc_params, kff) == 8 * 193 &&
            offsetof(qc_params, kp_p) == 8 * 199 && offsetof(qc_params, kd_w) == 8 * 208,
        "the groups sit where the record's table assumes them");
  bool scalar_used[31] = {};
  for (int e = 0; e < PARAM_COUNT; e++) {
    const int a = param_factor_a(e), b = param_factor_b(e);
    CHECK(a >= 0 && a < PARAM_RECORD && b >= 0 && b < PARAM_RECORD, "entry %d reads inside the record", e);
    if (e < 13 || e >= 193) {
      CHECK(b == 31 && a < 31 && !scalar_used[a], "entry %d is its own scalar times the 1", e);
      scalar_used[a] = true;
    } else if (e < 49) {
      CHECK(a == 32 + (e - 13) / 6 && b == 38 + (e - 13) % 6, "S entry %d = (-2 A z)[row] u[col]", e);
    } else {
      CHECK(a == 44 + (e - 49) / 12 && b == 56 + (e - 49) % 12, "W entry %d = (-2 z)[row] f[col]", e);
    }
  }
  for (int k = 0; k < 31; k++) CHECK(scalar_used[k], "scalar slot %d is read by an entry", k);
  CHECK(PARAM_RECORD_STRIDE >= PARAM_RECORD && PARAM_RECORD_STRIDE % 2 == 1, "an odd stride that holds the record");
  CHECK(PARAM_ENTRIES_PER_LANE * 64 >= PARAM_COUNT, "64 lanes cover the entries");
}

int main() {
  arguments();
  grid();
  layout();
  std::printf("sensitivity params host logic ok (%ld checks)\n", g_checked);
  return 0;
}
