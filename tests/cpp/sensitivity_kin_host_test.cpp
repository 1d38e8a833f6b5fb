// The device-free host logic of the joint-angle-cotangent entry point (quadruped_control_amd/csrc/qc_host.hpp):
// check_sensitivity_kin_args through every refusal of qc_sensitivity_kin_batch and the accepted combinations of its optional arrays.
// Host compiler only - links neither HIP nor the library; built with the address and undefined-behaviour sanitizers
// (__graft_entry__.build_host_test) and run by tests/test_sensitivity_kinematics_cpu.py.  Prints the failing case and exits 1 on the
// first violated check.
#include <cstdio>
#include <cstdlib>
#include <string>

#include "host_check.hpp"

using namespace qc;

static double buf[4];
static int32_t words[4];
static uint8_t bytes[4];

static qc_batch_in valid_in() {
  qc_batch_in in{};
  in.joint_q = buf;  // all the kernel reads besides the contact mask: no state array is required
  return in;
}
static qc_sensitivity_kin_io valid_io() {
  qc_sensitivity_kin_io io{};
  io.struct_size = sizeof(qc_sensitivity_kin_io);
  io.grf_body = buf;
  io.status = words;
  io.joint_tau_bar = buf;
  io.grf_bar = buf;
  return io;
}

static void arguments() {
  const qc_handle* const h = reinterpret_cast<const qc_handle*>(buf);  // only compared with null
  const qc_batch_in in = valid_in();
  const qc_sensitivity_kin_io io = valid_io();
  CHECK(check_sensitivity_kin_args(h, 1, &in, &io) == QC_OK, "the torque half: joint_tau_bar -> grf_bar, no state array in the batch");
  {
    qc_batch_in b = in;
    b.Rwb = b.Rwb_d = b.x = b.xdot = b.w = b.x_d = b.xdot_d = b.w_d = b.feet = buf;
    b.stance = bytes; b.gait_phase = buf; b.gait_duty = buf;
    b.gait_dt = buf; b.swing_pos = b.swing_vel = b.joint_qdot = buf;  // ignored, not refused
    qc_sensitivity_kin_io c = io;
    c.feet_bar = c.grf_bar_in = c.joint_q_bar_in = buf;
    c.joint_q_bar = buf;
    CHECK(check_sensitivity_kin_args(h, 4097, &b, &c) == QC_OK, "every array of the batch, every input and both outputs");
  }
  {
    qc_sensitivity_kin_io c{};
    c.struct_size = sizeof(qc_sensitivity_kin_io);
    c.feet_bar = buf; c.joint_q_bar = buf;
    CHECK(check_sensitivity_kin_args(h, 1, &in, &c) == QC_OK, "the kinematics half alone: feet_bar -> joint_q_bar, no grf_body, no status");
    c.joint_q_bar_in = buf;
    CHECK(check_sensitivity_kin_args(h, 1, &in, &c) == QC_OK, "the kinematics half on top of joint_q_bar_in");
    c.feet_bar = nullptr;
    CHECK(check_sensitivity_kin_args(h, 1, &in, &c) == QC_OK, "joint_q_bar_in alone");
    c.joint_q_bar_in = nullptr;
    c.joint_tau_bar = buf; c.grf_body = buf; c.status = words;
    CHECK(check_sensitivity_kin_args(h, 1, &in, &c) == QC_OK, "joint_tau_bar -> joint_q_bar alone");
    c.grf_bar_in = buf;
    CHECK(check_sensitivity_kin_args(h, 1, &in, &c) == QC_OK, "a grf_bar_in nobody asks the sum of is ignored");
  }
  const char* const null_arg = "qc_sensitivity_kin_batch: null argument";
  CHECK_FAILS(check_sensitivity_kin_args(nullptr, 1, &in, &io), null_arg, "no handle");
  CHECK_FAILS(check_sensitivity_kin_args(h, 1, nullptr, &io), null_arg, "no in");
  CHECK_FAILS(check_sensitivity_kin_args(h, 1, &in, nullptr), null_arg, "no io");
  CHECK_FAILS(check_sensitivity_kin_args(nullptr, 0, &in, &io), null_arg, "no handle, n = 0");
  for (const size_t sz : {(size_t)0, sizeof(qc_sensitivity_kin_io) - 8, sizeof(qc_sensitivity_kin_io) + 8, sizeof(qc_sensitivity_io)}) {
    qc_sensitivity_kin_io c = io;
    c.struct_size = sz;
    char text[320];
    std::snprintf(text, sizeof text,
                  "qc_sensitivity_kin_batch: qc_sensitivity_kin_io.struct_size is %zu, this library's qc_sensitivity_kin_io has %zu B (qc_default_sensitivity_kin sets it)",
                  sz, sizeof(qc_sensitivity_kin_io));
    CHECK_FAILS(check_sensitivity_kin_args(h, 1, &in, &c), text, "struct_size %zu", sz);
    CHECK_FAILS(check_sensitivity_kin_args(h, 0, &in, &c), text, "struct_size %zu, n = 0", sz);
  }
  {
    qc_sensitivity_kin_io c = io;
    c.grf_bar = nullptr;
    const char* const none = "qc_sensitivity_kin_batch: no output requested (grf_bar and joint_q_bar are both NULL)";
    CHECK_FAILS(check_sensitivity_kin_args(h, 1, &in, &c), none, "no output");
    CHECK_FAILS(check_sensitivity_kin_args(h, 0, &in, &c), none, "no output, n = 0");
    c.joint_q_bar = buf;
    CHECK(check_sensitivity_kin_args(h, 1, &in, &c) == QC_OK, "joint_q_bar alone");
  }
  {
    qc_sensitivity_kin_io c = io;
    c.joint_tau_bar = nullptr;
    c.grf_bar = nullptr; c.joint_q_bar = buf;
    const char* const none = "qc_sensitivity_kin_batch: no cotangent given (joint_tau_bar, feet_bar and joint_q_bar_in are all NULL)";
    CHECK_FAILS(check_sensitivity_kin_args(h, 1, &in, &c), none, "no cotangent");
    CHECK_FAILS(check_sensitivity_kin_args(h, 0, &in, &c), none, "no cotangent, n = 0");
    c.grf_bar_in = buf;
    CHECK_FAILS(check_sensitivity_kin_args(h, 1, &in, &c), none, "grf_bar_in is no cotangent of its own");
  }
  const char* const needs = "qc_sensitivity_kin_batch: joint_tau_bar needs grf_body and status";
  {
    qc_sensitivity_kin_io c = io;
    c.grf_body = nullptr;
    CHECK_FAILS(check_sensitivity_kin_args(h, 1, &in, &c), needs, "joint_tau_bar without grf_body");
    CHECK_FAILS(check_sensitivity_kin_args(h, 0, &in, &c), needs, "joint_tau_bar without grf_body, n = 0");
    c = io;
    c.status = nullptr;
    CHECK_FAILS(check_sensitivity_kin_args(h, 1, &in, &c), needs, "joint_tau_bar without status");
  }
  {
    qc_sensitivity_kin_io c = io;
    c.joint_tau_bar = nullptr;
    c.feet_bar = buf;
    const char* const text = "qc_sensitivity_kin_batch: grf_bar needs joint_tau_bar";
    CHECK_FAILS(check_sensitivity_kin_args(h, 1, &in, &c), text, "grf_bar without joint_tau_bar");
    c.joint_q_bar = buf;
    CHECK_FAILS(check_sensitivity_kin_args(h, 1, &in, &c), text, "grf_bar without joint_tau_bar, next to joint_q_bar");
  }
  {
    qc_batch_in b = in;
    b.joint_q = nullptr;
    b.feet = buf;  // `feet` is not this path
    CHECK_FAILS(check_sensitivity_kin_args(h, 1, &b, &io), "qc_sensitivity_kin_batch: joint_q is required", "no joint_q");
    CHECK(check_sensitivity_kin_args(h, 0, &b, &io) == QC_OK, "no joint_q, n = 0 asks for no array");
  }
  const size_t most = (size_t)0xFFFFFF * SENSITIVITY_BLOCK;
  CHECK(check_sensitivity_kin_args(h, most, &in, &io) == QC_OK, "the largest batch of one launch");
  CHECK_FAILS(check_sensitivity_kin_args(h, most + 1, &in, &io), "qc_sensitivity_kin_batch: n is beyond one launch", "one robot more");
  CHECK(sensitivity_kin_blocks(1) == 1 && sensitivity_kin_blocks(16) == 1 && sensitivity_kin_blocks(17) == 2, "a workgroup holds the legs of 16 robots");
  CHECK(sensitivity_kin_blocks(most) == (unsigned)SENSITIVITY_MAX_BLOCKS, "the grid is capped: the waves stride");
  CHECK(sizeof(qc_sensitivity_kin_io) == 9 * 8, "the io record: struct_size, six inputs and two outputs");
  CHECK(sizeof(qc_sensitivity_io) == 14 * 8 && sizeof(qc_sensitivity_rot_io) == 9 * 8, "the neighbours keep their size");
}

int main() {
  arguments();
  std::printf("sensitivity kinematics host logic ok (%ld checks)\n", g_checked);
  return 0;
}
