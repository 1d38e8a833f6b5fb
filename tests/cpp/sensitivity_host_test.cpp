// The device-free host logic of the sensitivity entry point (quadruped_control_amd/csrc/qc_host.hpp): check_sensitivity_args
// through every refusal of qc_sensitivity_batch, and the grid the entry point launches.  Host compiler only - links neither HIP
// nor the library; built with the address and undefined-behaviour sanitizers (__graft_entry__.build_sensitivity_host_test) and
// run by tests/test_sensitivity_cpu.py.  Prints the failing case and exits 1 on the first violated check.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <string>

#include "host_check.hpp"

using namespace qc;

static const double kInf = std::numeric_limits<double>::infinity();
static const double kNan = std::numeric_limits<double>::quiet_NaN();

static double buf[4];
static uint8_t bytes[4];
static int32_t word;

static qc_batch_in valid_in() {
  qc_batch_in in{};
  in.Rwb = in.Rwb_d = in.x = in.xdot = in.w = in.x_d = in.xdot_d = in.w_d = in.feet = buf;
  return in;
}
static qc_sensitivity_io valid_io() {
  qc_sensitivity_io io{};
  io.struct_size = sizeof(qc_sensitivity_io);
  io.grf_body = io.grf_bar = buf;
  io.act_tol = 1e-7;
  io.adjoint = buf;
  return io;
}

static void arguments() {
  const qc_handle* const h = reinterpret_cast<const qc_handle*>(buf);  // only compared with null
  const qc_batch_in in = valid_in();
  const qc_sensitivity_io io = valid_io();
  CHECK(check_sensitivity_args(h, 1, &in, &io) == QC_OK, "the smallest valid call (one output)");
  {
    qc_batch_in b = in;
    b.feet = nullptr; b.joint_q = buf; b.stance = bytes; b.gait_phase = buf; b.gait_duty = buf;
    b.gait_dt = buf; b.swing_pos = b.swing_vel = b.joint_qdot = buf;  // ignored, not refused
    qc_sensitivity_io c = io;
    c.b_bar = c.feet_bar = c.x_bar = c.xdot_bar = c.w_bar = c.x_d_bar = c.xdot_d_bar = c.w_d_bar = buf; c.flags = &word;
    CHECK(check_sensitivity_args(h, 4097, &b, &c) == QC_OK, "joint_q, every optional input and every output");
  }
  const char* const null_arg = "qc_sensitivity_batch: null argument";
  CHECK_FAILS(check_sensitivity_args(nullptr, 1, &in, &io), null_arg, "no handle");
  CHECK_FAILS(check_sensitivity_args(h, 1, nullptr, &io), null_arg, "no in");
  CHECK_FAILS(check_sensitivity_args(h, 1, &in, nullptr), null_arg, "no io");
  CHECK_FAILS(check_sensitivity_args(nullptr, 0, &in, &io), null_arg, "no handle, n = 0");
  for (const size_t sz : {(size_t)0, sizeof(qc_sensitivity_io) - 8, sizeof(qc_sensitivity_io) + 8, sizeof(qc_certify_io)}) {
    qc_sensitivity_io c = io;
    c.struct_size = sz;
    char text[224];
    std::snprintf(text, sizeof(text),
                  "qc_sensitivity_batch: qc_sensitivity_io.struct_size is %zu, this library's qc_sensitivity_io has %zu B (qc_default_sensitivity sets it)", sz,
                  sizeof(qc_sensitivity_io));
    CHECK_FAILS(check_sensitivity_args(h, 1, &in, &c), text, "struct_size %zu", sz);
    CHECK_FAILS(check_sensitivity_args(h, 0, &in, &c), text, "struct_size %zu, n = 0", sz);
  }
  const char* const tol = "qc_sensitivity_batch: act_tol must be finite and >= 0";
  for (const double bad : {-1e-300, -1.0, kInf, -kInf, kNan}) {
    qc_sensitivity_io c = io;
    c.act_tol = bad;
    CHECK_FAILS(check_sensitivity_args(h, 1, &in, &c), tol, "act_tol = %g", bad);
    CHECK_FAILS(check_sensitivity_args(h, 0, &in, &c), tol, "act_tol = %g, n = 0", bad);
  }
  {
    qc_sensitivity_io c = io;
    c.act_tol = 0.0;
    CHECK(check_sensitivity_args(h, 1, &in, &c) == QC_OK, "a zero tolerance is allowed");
  }
  {
    qc_sensitivity_io c = io;
    c.adjoint = nullptr;
    const char* const none =
        "qc_sensitivity_batch: no output requested (adjoint, b_bar, feet_bar, x_bar, xdot_bar, w_bar, x_d_bar, xdot_d_bar, w_d_bar, flags are all NULL)";
    CHECK_FAILS(check_sensitivity_args(h, 1, &in, &c), none, "no output");
    CHECK_FAILS(check_sensitivity_args(h, 0, &in, &c), none, "no output, n = 0");
    // each output alone is enough
    double* qc_sensitivity_io::* const outs[] = {&qc_sensitivity_io::b_bar,  &qc_sensitivity_io::feet_bar, &qc_sensitivity_io::x_bar,
                                                 &qc_sensitivity_io::xdot_bar, &qc_sensitivity_io::w_bar,  &qc_sensitivity_io::x_d_bar,
                                                 &qc_sensitivity_io::xdot_d_bar, &qc_sensitivity_io::w_d_bar};
    for (size_t m = 0; m < sizeof(outs) / sizeof(outs[0]); m++) {
      c = io; c.adjoint = nullptr; c.*outs[m] = buf;
      CHECK(check_sensitivity_args(h, 1, &in, &c) == QC_OK, "output %zu alone", m);
    }
    c = io; c.adjoint = nullptr; c.flags = &word;
    CHECK(check_sensitivity_args(h, 1, &in, &c) == QC_OK, "flags alone");
  }
  const char* const forces = "qc_sensitivity_batch: grf_body and grf_bar are required";
  {
    qc_sensitivity_io c = io;
    c.grf_body = nullptr;
    CHECK_FAILS(check_sensitivity_args(h, 1, &in, &c), forces, "no grf_body");
    CHECK(check_sensitivity_args(h, 0, &in, &c) == QC_OK, "n = 0 asks for no array");
    c = io;
    c.grf_bar = nullptr;
    CHECK_FAILS(check_sensitivity_args(h, 1, &in, &c), forces, "no grf_bar");
    CHECK(check_sensitivity_args(h, 0, &in, &c) == QC_OK, "n = 0 asks for no cotangent");
  }
  const char* const state =
      "qc_sensitivity_batch: the state arrays Rwb, Rwb_d, x, xdot, w, x_d, xdot_d and w_d are required (commander mode is out of scope)";
  const double* qc_batch_in::* const members[] = {&qc_batch_in::Rwb, &qc_batch_in::Rwb_d, &qc_batch_in::x, &qc_batch_in::xdot,
                                                  &qc_batch_in::w, &qc_batch_in::x_d, &qc_batch_in::xdot_d, &qc_batch_in::w_d};
  for (size_t m = 0; m < sizeof(members) / sizeof(members[0]); m++) {
    qc_batch_in b = in;
    b.*members[m] = nullptr;
    CHECK_FAILS(check_sensitivity_args(h, 1, &b, &io), state, "state array %zu missing", m);
    CHECK(check_sensitivity_args(h, 0, &b, &io) == QC_OK, "state array %zu missing, n = 0", m);
  }
  {
    qc_batch_in b = in;
    b.feet = nullptr;
    CHECK_FAILS(check_sensitivity_args(h, 1, &b, &io), "qc_sensitivity_batch: feet or joint_q is required", "neither feet nor joint_q");
    b.joint_q = buf;
    CHECK(check_sensitivity_args(h, 1, &b, &io) == QC_OK, "joint_q in place of feet");
  }
  const size_t most = (size_t)0xFFFFFF * SENSITIVITY_BLOCK;
  CHECK(check_sensitivity_args(h, most, &in, &io) == QC_OK, "the largest batch of one launch");
  CHECK_FAILS(check_sensitivity_args(h, most + 1, &in, &io), "qc_sensitivity_batch: n is beyond one launch", "one robot more");
}

static void grid() {
  CHECK(sensitivity_blocks(1) == 1 && sensitivity_blocks(64) == 1 && sensitivity_blocks(65) == 2 && sensitivity_blocks(130) == 3 &&
            sensitivity_blocks(1000) == 16,
        "one wave per 64 robots");
  const size_t cap = (size_t)SENSITIVITY_MAX_BLOCKS * SENSITIVITY_BLOCK;
  CHECK(sensitivity_blocks(cap) == (unsigned)SENSITIVITY_MAX_BLOCKS && sensitivity_blocks(cap + 1) == (unsigned)SENSITIVITY_MAX_BLOCKS &&
            sensitivity_blocks((size_t)0xFFFFFF * SENSITIVITY_BLOCK) == (unsigned)SENSITIVITY_MAX_BLOCKS,
        "the grid is capped: the waves stride beyond it");
  CHECK(sizeof(qc_sensitivity_io) == 14 * 8, "the io record: struct_size, two inputs, act_tol and ten outputs");
}

int main() {
  arguments();
  grid();
  std::printf("sensitivity host logic ok (%ld checks)\n", g_checked);
  return 0;
}
