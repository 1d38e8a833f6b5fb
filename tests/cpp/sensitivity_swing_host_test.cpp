// The device-free host logic of the swing-leg torque adjoint's entry point (quadruped_control_amd/csrc/qc_host.hpp):
// check_sensitivity_swing_args through every refusal of qc_sensitivity_swing_batch and the accepted combinations of its optional arrays.
// Host compiler only - links neither HIP nor the library; built with the address and undefined-behaviour sanitizers
// (__graft_entry__.build_host_test) and run by tests/test_sensitivity_swing_cpu.py.  Prints the failing case and exits 1 on the
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
  in.Rwb = in.x = in.joint_q = in.joint_qdot = in.swing_pos = in.swing_vel = buf;  // the six arrays of the swing chain
  return in;
}
static qc_sensitivity_swing_io valid_io() {
  qc_sensitivity_swing_io io{};
  io.struct_size = sizeof(qc_sensitivity_swing_io);
  io.joint_tau_bar = buf;
  io.joint_q_bar = buf;
  return io;
}

static void arguments() {
  const qc_handle* const h = reinterpret_cast<const qc_handle*>(buf);  // only compared with null
  const qc_batch_in in = valid_in();
  const qc_sensitivity_swing_io io = valid_io();
  CHECK(check_sensitivity_swing_args(h, 1, &in, &io) == QC_OK, "joint_tau_bar -> joint_q_bar, no contact array: all stance");
  {
    qc_batch_in b = in;
    b.Rwb_d = b.xdot = b.w = b.x_d = b.xdot_d = b.w_d = b.feet = buf;  // ignored, not refused
    b.stance = bytes; b.gait_phase = buf; b.gait_duty = buf;
    qc_sensitivity_swing_io c = io;
    c.joint_q_bar_in = c.Rwb_bar_in = c.x_bar_in = buf;
    c.swing_pos_bar = c.swing_vel_bar = c.joint_qdot_bar = c.gain_bar = c.Rwb_bar = c.x_bar = buf;
    c.flags = words;
    CHECK(check_sensitivity_swing_args(h, 4097, &b, &c) == QC_OK, "every array of the batch but the refused two, every input and every output");
  }
  {  // every output alone, with and without the accumulators
    double* qc_sensitivity_swing_io::* const outs[] = {&qc_sensitivity_swing_io::swing_pos_bar, &qc_sensitivity_swing_io::swing_vel_bar,
                                                       &qc_sensitivity_swing_io::joint_q_bar,   &qc_sensitivity_swing_io::joint_qdot_bar,
                                                       &qc_sensitivity_swing_io::gain_bar,      &qc_sensitivity_swing_io::Rwb_bar,
                                                       &qc_sensitivity_swing_io::x_bar};
    int k = 0;
    for (const auto m : outs) {
      qc_sensitivity_swing_io c{};
      c.struct_size = sizeof(qc_sensitivity_swing_io);
      c.joint_tau_bar = buf;
      c.*m = buf;
      CHECK(check_sensitivity_swing_args(h, 1, &in, &c) == QC_OK, "output %d alone", k);
      c.joint_q_bar_in = c.Rwb_bar_in = c.x_bar_in = buf;
      CHECK(check_sensitivity_swing_args(h, 1, &in, &c) == QC_OK, "output %d alone, every accumulator given (one nobody asks the sum of is ignored)", k);
      k++;
    }
    qc_sensitivity_swing_io c{};
    c.struct_size = sizeof(qc_sensitivity_swing_io);
    c.joint_tau_bar = buf;
    c.flags = words;
    CHECK(check_sensitivity_swing_args(h, 1, &in, &c) == QC_OK, "flags alone count as an output");
  }
  {
    qc_batch_in b = in;
    b.stance = bytes;
    CHECK(check_sensitivity_swing_args(h, 1, &b, &io) == QC_OK, "the mask from stance bytes");
    b.stance = nullptr; b.gait_phase = buf;
    CHECK(check_sensitivity_swing_args(h, 1, &b, &io) == QC_OK, "the mask from the phases, the handle's duty");
    b.gait_duty = buf;
    CHECK(check_sensitivity_swing_args(h, 1, &b, &io) == QC_OK, "the mask from the phases and a duty per robot");
  }
  const char* const null_arg = "qc_sensitivity_swing_batch: null argument";
  CHECK_FAILS(check_sensitivity_swing_args(nullptr, 1, &in, &io), null_arg, "no handle");
  CHECK_FAILS(check_sensitivity_swing_args(h, 1, nullptr, &io), null_arg, "no in");
  CHECK_FAILS(check_sensitivity_swing_args(h, 1, &in, nullptr), null_arg, "no io");
  CHECK_FAILS(check_sensitivity_swing_args(nullptr, 0, &in, &io), null_arg, "no handle, n = 0");
  for (const size_t sz : {(size_t)0, sizeof(qc_sensitivity_swing_io) - 8, sizeof(qc_sensitivity_swing_io) + 8, sizeof(qc_sensitivity_kin_io)}) {
    qc_sensitivity_swing_io c = io;
    c.struct_size = sz;
    char text[320];
    std::snprintf(text, sizeof text,
                  "qc_sensitivity_swing_batch: qc_sensitivity_swing_io.struct_size is %zu, this library's qc_sensitivity_swing_io has %zu B (qc_default_sensitivity_swing sets it)",
                  sz, sizeof(qc_sensitivity_swing_io));
    CHECK_FAILS(check_sensitivity_swing_args(h, 1, &in, &c), text, "struct_size %zu", sz);
    CHECK_FAILS(check_sensitivity_swing_args(h, 0, &in, &c), text, "struct_size %zu, n = 0", sz);
  }
  {
    qc_batch_in b = in;
    b.swing_state = reinterpret_cast<qc_swing_state*>(buf);
    const char* const text = "qc_sensitivity_swing_batch: swing_state must be NULL (the planner's references are out of scope: give swing_pos and swing_vel)";
    CHECK_FAILS(check_sensitivity_swing_args(h, 1, &b, &io), text, "swing_state");
    CHECK_FAILS(check_sensitivity_swing_args(h, 0, &b, &io), text, "swing_state, n = 0");
    b.gait_dt = buf;
    CHECK_FAILS(check_sensitivity_swing_args(h, 1, &b, &io), text, "swing_state and gait_dt: swing_state is named");
  }
  {
    qc_batch_in b = in;
    b.gait_phase = buf; b.gait_dt = buf;
    const char* const text = "qc_sensitivity_swing_batch: gait_dt must be NULL (the gait clock is out of scope: the contact mask is read as it is now)";
    CHECK_FAILS(check_sensitivity_swing_args(h, 1, &b, &io), text, "gait_dt");
    CHECK_FAILS(check_sensitivity_swing_args(h, 0, &b, &io), text, "gait_dt, n = 0");
  }
  {
    qc_sensitivity_swing_io c = io;
    c.joint_q_bar = nullptr;
    const char* const none =
        "qc_sensitivity_swing_batch: no output requested (swing_pos_bar, swing_vel_bar, joint_q_bar, joint_qdot_bar, gain_bar, Rwb_bar, x_bar, flags are all NULL)";
    CHECK_FAILS(check_sensitivity_swing_args(h, 1, &in, &c), none, "no output");
    CHECK_FAILS(check_sensitivity_swing_args(h, 0, &in, &c), none, "no output, n = 0");
    c.joint_q_bar_in = c.Rwb_bar_in = c.x_bar_in = buf;
    CHECK_FAILS(check_sensitivity_swing_args(h, 1, &in, &c), none, "the accumulators are no outputs");
  }
  {
    qc_sensitivity_swing_io c = io;
    c.joint_tau_bar = nullptr;
    CHECK_FAILS(check_sensitivity_swing_args(h, 1, &in, &c), "qc_sensitivity_swing_batch: joint_tau_bar is required", "no joint_tau_bar");
    CHECK(check_sensitivity_swing_args(h, 0, &in, &c) == QC_OK, "no joint_tau_bar, n = 0 asks for no array");
  }
  {
    const double* qc_batch_in::* const six[] = {&qc_batch_in::Rwb, &qc_batch_in::x, &qc_batch_in::joint_q, &qc_batch_in::joint_qdot, &qc_batch_in::swing_pos,
                                                &qc_batch_in::swing_vel};
    int k = 0;
    for (const auto m : six) {
      qc_batch_in b = in;
      b.*m = nullptr;
      b.feet = buf;  // `feet` is not this path
      CHECK_FAILS(check_sensitivity_swing_args(h, 1, &b, &io), "qc_sensitivity_swing_batch: Rwb, x, joint_q, joint_qdot, swing_pos and swing_vel are required",
                  "input %d missing", k);
      CHECK(check_sensitivity_swing_args(h, 0, &b, &io) == QC_OK, "input %d missing, n = 0 asks for no array", k);
      k++;
    }
  }
  const size_t most = (size_t)0xFFFFFF * SENSITIVITY_BLOCK;
  CHECK(check_sensitivity_swing_args(h, most, &in, &io) == QC_OK, "the largest batch of one launch");
  CHECK_FAILS(check_sensitivity_swing_args(h, most + 1, &in, &io), "qc_sensitivity_swing_batch: n is beyond one launch", "one robot more");
  CHECK(sensitivity_swing_blocks(1) == 1 && sensitivity_swing_blocks(16) == 1 && sensitivity_swing_blocks(17) == 2, "a workgroup holds the legs of 16 robots");
  CHECK(sensitivity_swing_blocks(most) == (unsigned)SENSITIVITY_MAX_BLOCKS, "the grid is capped: the waves stride");
  CHECK(sizeof(qc_sensitivity_swing_io) == 13 * 8, "the io record: struct_size, four inputs and eight outputs");
  CHECK(sizeof(qc_sensitivity_kin_io) == 9 * 8 && sizeof(qc_sensitivity_rot_io) == 9 * 8, "the neighbours keep their size");
}

int main() {
  arguments();
  std::printf("sensitivity swing host logic ok (%ld checks)\n", g_checked);
  return 0;
}
