// The device-free host logic of the rotation-cotangent entry point (quadruped_control_amd/csrc/qc_host.hpp):
// check_sensitivity_rot_args through every refusal of qc_sensitivity_rot_batch.  Host compiler only - links neither HIP nor the
// library; built with the address and undefined-behaviour sanitizers (__graft_entry__.build_host_test) and run by
// tests/test_sensitivity_rotation_cpu.py.  Prints the failing case and exits 1 on the first violated check.
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
static qc_sensitivity_rot_io valid_io() {
  qc_sensitivity_rot_io io{};
  io.struct_size = sizeof(qc_sensitivity_rot_io);
  io.grf_body = io.grf_bar = io.b_bar = io.feet_bar = buf;
  io.Rwb_bar = buf;
  return io;
}

static void arguments() {
  const qc_handle* const h = reinterpret_cast<const qc_handle*>(buf);  // only compared with null
  const qc_batch_in in = valid_in();
  const qc_sensitivity_rot_io io = valid_io();
  CHECK(check_sensitivity_rot_args(h, 1, &in, &io) == QC_OK, "the smallest valid call (one output)");
  {
    qc_batch_in b = in;
    b.feet = nullptr; b.joint_q = buf; b.stance = bytes; b.gait_phase = buf; b.gait_duty = buf;
    b.gait_dt = buf; b.swing_pos = b.swing_vel = b.joint_qdot = buf;  // ignored, not refused
    qc_sensitivity_rot_io c = io;
    c.Rwb_d_bar = c.Rwb_rot_bar = c.Rwb_d_rot_bar = buf;
    CHECK(check_sensitivity_rot_args(h, 4097, &b, &c) == QC_OK, "joint_q, every optional input and every output");
  }
  const char* const null_arg = "qc_sensitivity_rot_batch: null argument";
  CHECK_FAILS(check_sensitivity_rot_args(nullptr, 1, &in, &io), null_arg, "no handle");
  CHECK_FAILS(check_sensitivity_rot_args(h, 1, nullptr, &io), null_arg, "no in");
  CHECK_FAILS(check_sensitivity_rot_args(h, 1, &in, nullptr), null_arg, "no io");
  CHECK_FAILS(check_sensitivity_rot_args(nullptr, 0, &in, &io), null_arg, "no handle, n = 0");
  for (const size_t sz : {(size_t)0, sizeof(qc_sensitivity_rot_io) - 8, sizeof(qc_sensitivity_rot_io) + 8, sizeof(qc_sensitivity_io)}) {
    qc_sensitivity_rot_io c = io;
    c.struct_size = sz;
    char text[320];
    std::snprintf(text, sizeof text,
                  "qc_sensitivity_rot_batch: qc_sensitivity_rot_io.struct_size is %zu, this library's qc_sensitivity_rot_io has %zu B (qc_default_sensitivity_rot sets it)",
                  sz, sizeof(qc_sensitivity_rot_io));
    CHECK_FAILS(check_sensitivity_rot_args(h, 1, &in, &c), text, "struct_size %zu", sz);
    CHECK_FAILS(check_sensitivity_rot_args(h, 0, &in, &c), text, "struct_size %zu, n = 0", sz);
  }
  double* qc_sensitivity_rot_io::* const outs[] = {&qc_sensitivity_rot_io::Rwb_bar, &qc_sensitivity_rot_io::Rwb_d_bar, &qc_sensitivity_rot_io::Rwb_rot_bar,
                                                   &qc_sensitivity_rot_io::Rwb_d_rot_bar};
  {
    qc_sensitivity_rot_io c = io;
    c.Rwb_bar = nullptr;
    const char* const none = "qc_sensitivity_rot_batch: no output requested (Rwb_bar, Rwb_d_bar, Rwb_rot_bar, Rwb_d_rot_bar are all NULL)";
    CHECK_FAILS(check_sensitivity_rot_args(h, 1, &in, &c), none, "no output");
    CHECK_FAILS(check_sensitivity_rot_args(h, 0, &in, &c), none, "no output, n = 0");
    for (size_t m = 0; m < sizeof(outs) / sizeof(outs[0]); m++) {
      qc_sensitivity_rot_io one = c;
      one.*outs[m] = buf;
      CHECK(check_sensitivity_rot_args(h, 1, &in, &one) == QC_OK, "output %zu alone", m);
    }
  }
  const char* const inputs = "qc_sensitivity_rot_batch: grf_body, grf_bar, b_bar and feet_bar are required";
  const double* qc_sensitivity_rot_io::* const ins[] = {&qc_sensitivity_rot_io::grf_body, &qc_sensitivity_rot_io::grf_bar, &qc_sensitivity_rot_io::b_bar,
                                                        &qc_sensitivity_rot_io::feet_bar};
  for (size_t m = 0; m < sizeof(ins) / sizeof(ins[0]); m++) {
    qc_sensitivity_rot_io c = io;
    c.*ins[m] = nullptr;
    CHECK_FAILS(check_sensitivity_rot_args(h, 1, &in, &c), inputs, "input %zu missing", m);
    CHECK(check_sensitivity_rot_args(h, 0, &in, &c) == QC_OK, "input %zu missing, n = 0 asks for no array", m);
  }
  const char* const state =
      "qc_sensitivity_rot_batch: the state arrays Rwb, Rwb_d, x, xdot, w, x_d, xdot_d and w_d are required (commander mode is out of scope)";
  const double* qc_batch_in::* const members[] = {&qc_batch_in::Rwb, &qc_batch_in::Rwb_d, &qc_batch_in::x, &qc_batch_in::xdot,
                                                  &qc_batch_in::w, &qc_batch_in::x_d, &qc_batch_in::xdot_d, &qc_batch_in::w_d};
  for (size_t m = 0; m < sizeof(members) / sizeof(members[0]); m++) {
    qc_batch_in b = in;
    b.*members[m] = nullptr;
    CHECK_FAILS(check_sensitivity_rot_args(h, 1, &b, &io), state, "state array %zu missing", m);
    CHECK(check_sensitivity_rot_args(h, 0, &b, &io) == QC_OK, "state array %zu missing, n = 0", m);
  }
  {
    // commander mode keeps Rwb_d, x_d, xdot_d and w_d in its own record and leaves them NULL in qc_batch_in: refused as a whole
    qc_batch_in b = in;
    b.Rwb_d = b.x_d = b.xdot_d = b.w_d = nullptr;
    b.feet = nullptr; b.joint_q = buf;
    CHECK_FAILS(check_sensitivity_rot_args(h, 1, &b, &io), state, "a commander-mode batch");
  }
  {
    qc_batch_in b = in;
    b.feet = nullptr;
    CHECK_FAILS(check_sensitivity_rot_args(h, 1, &b, &io), "qc_sensitivity_rot_batch: feet or joint_q is required", "neither feet nor joint_q");
    b.joint_q = buf;
    CHECK(check_sensitivity_rot_args(h, 1, &b, &io) == QC_OK, "joint_q in place of feet");
  }
  const size_t most = (size_t)0xFFFFFF * SENSITIVITY_BLOCK;
  CHECK(check_sensitivity_rot_args(h, most, &in, &io) == QC_OK, "the largest batch of one launch");
  CHECK_FAILS(check_sensitivity_rot_args(h, most + 1, &in, &io), "qc_sensitivity_rot_batch: n is beyond one launch", "one robot more");
  CHECK(sizeof(qc_sensitivity_rot_io) == 9 * 8, "the io record: struct_size, four inputs and four outputs");
  CHECK(sizeof(qc_sensitivity_io) == 14 * 8, "qc_sensitivity_io keeps its size");
}

int main() {
  arguments();
  std::printf("sensitivity rotation host logic ok (%ld checks)\n", g_checked);
  return 0;
}
