// The device-free host logic of the swing references' two entry points (quadruped_control_amd/csrc/qc_host.hpp):
// check_swing_reference_args and check_swing_reference_adjoint_args through every refusal of qc_swing_reference_batch and
// qc_swing_reference_adjoint_batch and the accepted combinations of their optional arrays.
// Host compiler only - links neither HIP nor the library; built with the address and undefined-behaviour sanitizers
// (__graft_entry__.build_host_test) and run by tests/test_swing_reference_cpu.py.  Prints the failing case and exits 1 on the
// first violated check.
#include <cstdio>
#include <cstdlib>
#include <string>

#include "host_check.hpp"

using namespace qc;

static double buf[4];
static int32_t words[4];
static uint8_t bytes[4];
static qc_swing_state records[1];

static qc_batch_in valid_in() {
  qc_batch_in in{};
  in.Rwb = in.x = in.xdot = in.w = in.xdot_d = in.joint_q = buf;
  in.gait_phase = buf;
  in.swing_state = records;
  return in;
}

static void forward() {
  const qc_handle* const h = reinterpret_cast<const qc_handle*>(buf);  // only compared with null
  const qc_batch_in in = valid_in();
  qc_swing_reference_io io{};
  io.struct_size = sizeof(qc_swing_reference_io);
  io.swing_pos = buf;
  CHECK(check_swing_reference_args(h, 1, &in, &io) == QC_OK, "the eight required arrays -> swing_pos");
  {
    qc_batch_in b = in;
    b.Rwb_d = b.x_d = b.w_d = b.joint_qdot = b.feet = buf;  // ignored, not refused (feet WITH joint_q)
    b.gait_duty = b.gait_dt = buf;
    qc_swing_reference_io c = io;
    c.swing_vel = buf; c.planned = bytes;
    CHECK(check_swing_reference_args(h, 4097, &b, &c) == QC_OK, "the clock, a duty per robot, every output");
    b.gait_dt = nullptr; b.stance = bytes;
    CHECK(check_swing_reference_args(h, 1, &b, &c) == QC_OK, "the mask from stance bytes, no clock");
  }
  for (int k = 0; k < 3; k++) {
    qc_swing_reference_io c{};
    c.struct_size = sizeof(qc_swing_reference_io);
    if (k == 0) c.swing_pos = buf;
    if (k == 1) c.swing_vel = buf;
    if (k == 2) c.planned = bytes;
    CHECK(check_swing_reference_args(h, 1, &in, &c) == QC_OK, "output %d alone", k);
  }
  const char* const null_arg = "qc_swing_reference_batch: null argument";
  CHECK_FAILS(check_swing_reference_args(nullptr, 1, &in, &io), null_arg, "no handle");
  CHECK_FAILS(check_swing_reference_args(h, 1, nullptr, &io), null_arg, "no in");
  CHECK_FAILS(check_swing_reference_args(h, 1, &in, nullptr), null_arg, "no io");
  CHECK_FAILS(check_swing_reference_args(nullptr, 0, &in, &io), null_arg, "no handle, n = 0");
  for (const size_t sz : {(size_t)0, sizeof(qc_swing_reference_io) - 8, sizeof(qc_swing_reference_io) + 8, sizeof(qc_swing_reference_adjoint_io)}) {
    qc_swing_reference_io c = io;
    c.struct_size = sz;
    char text[320];
    std::snprintf(text, sizeof text,
                  "qc_swing_reference_batch: qc_swing_reference_io.struct_size is %zu, this library's qc_swing_reference_io has %zu B (qc_default_swing_reference sets it)",
                  sz, sizeof(qc_swing_reference_io));
    CHECK_FAILS(check_swing_reference_args(h, 1, &in, &c), text, "struct_size %zu", sz);
    CHECK_FAILS(check_swing_reference_args(h, 0, &in, &c), text, "struct_size %zu, n = 0", sz);
  }
  {
    const char* const text = "qc_swing_reference_batch: swing_pos and swing_vel must be NULL (this call makes them)";
    qc_batch_in b = in;
    b.swing_pos = buf;
    CHECK_FAILS(check_swing_reference_args(h, 1, &b, &io), text, "swing_pos given");
    CHECK_FAILS(check_swing_reference_args(h, 0, &b, &io), text, "swing_pos given, n = 0");
    b.swing_pos = nullptr; b.swing_vel = buf;
    CHECK_FAILS(check_swing_reference_args(h, 1, &b, &io), text, "swing_vel given");
  }
  {
    const char* const text = "qc_swing_reference_batch: feet without joint_q (the planner starts from the forward kinematics of joint_q)";
    qc_batch_in b = in;
    b.joint_q = nullptr; b.feet = buf;
    CHECK_FAILS(check_swing_reference_args(h, 1, &b, &io), text, "feet in place of joint_q");
    CHECK_FAILS(check_swing_reference_args(h, 0, &b, &io), text, "feet in place of joint_q, n = 0");
  }
  {
    const char* const text = "qc_swing_reference_batch: gait_dt advances gait_phase (stance must be NULL)";
    qc_batch_in b = in;
    b.gait_dt = buf; b.stance = bytes;
    CHECK_FAILS(check_swing_reference_args(h, 1, &b, &io), text, "gait_dt with stance");
    CHECK_FAILS(check_swing_reference_args(h, 0, &b, &io), text, "gait_dt with stance, n = 0");
  }
  {
    const char* const none = "qc_swing_reference_batch: no output requested (swing_pos, swing_vel, planned are all NULL)";
    qc_swing_reference_io c = io;
    c.swing_pos = nullptr;
    CHECK_FAILS(check_swing_reference_args(h, 1, &in, &c), none, "no output");
    CHECK_FAILS(check_swing_reference_args(h, 0, &in, &c), none, "no output, n = 0");
  }
  {
    const char* const text = "qc_swing_reference_batch: Rwb, x, xdot, w, xdot_d, joint_q, gait_phase and swing_state are required";
    const double* qc_batch_in::* const six[] = {&qc_batch_in::Rwb, &qc_batch_in::x, &qc_batch_in::xdot, &qc_batch_in::w, &qc_batch_in::xdot_d, &qc_batch_in::joint_q};
    int k = 0;
    for (const auto m : six) {
      qc_batch_in b = in;
      b.*m = nullptr;
      CHECK_FAILS(check_swing_reference_args(h, 1, &b, &io), text, "input %d missing", k);
      CHECK(check_swing_reference_args(h, 0, &b, &io) == QC_OK, "input %d missing, n = 0 asks for no array", k);
      k++;
    }
    qc_batch_in b = in;
    b.gait_phase = nullptr;
    CHECK_FAILS(check_swing_reference_args(h, 1, &b, &io), text, "no gait_phase");
    b = in;
    b.swing_state = nullptr;
    CHECK_FAILS(check_swing_reference_args(h, 1, &b, &io), text, "no swing_state");
    CHECK(check_swing_reference_args(h, 0, &b, &io) == QC_OK, "no swing_state, n = 0 asks for no array");
  }
  const size_t most = (size_t)0xFFFFFF * SENSITIVITY_BLOCK;
  CHECK(check_swing_reference_args(h, most, &in, &io) == QC_OK, "the largest batch of one launch");
  CHECK_FAILS(check_swing_reference_args(h, most + 1, &in, &io), "qc_swing_reference_batch: n is beyond one launch", "one robot more");
  CHECK(swing_reference_blocks(1) == 1 && swing_reference_blocks(64) == 1 && swing_reference_blocks(65) == 2, "a workgroup holds 64 robots");
  CHECK(swing_reference_blocks(most) == (unsigned)SENSITIVITY_MAX_BLOCKS, "the grid is capped: the waves stride");
  CHECK(sizeof(qc_swing_reference_io) == 4 * 8, "the io record: struct_size and three outputs");
}

static void adjoint() {
  const qc_handle* const h = reinterpret_cast<const qc_handle*>(buf);
  qc_batch_in in{};
  in.Rwb = in.x = in.xdot = in.w = in.joint_q = buf;
  in.gait_phase = buf;
  qc_swing_reference_adjoint_io io{};
  io.struct_size = sizeof(qc_swing_reference_adjoint_io);
  io.state_before = records;
  io.swing_pos_bar = buf;
  io.x_bar = buf;
  CHECK(check_swing_reference_adjoint_args(h, 1, &in, &io) == QC_OK, "swing_pos_bar -> x_bar");
  {
    qc_batch_in b = in;
    b.Rwb_d = b.x_d = b.xdot_d = b.w_d = b.joint_qdot = b.feet = b.gait_duty = buf;  // ignored, not refused
    b.swing_state = records;                                                         // the forward call's: not read here
    b.stance = bytes;
    qc_swing_reference_adjoint_io c = io;
    c.swing_vel_bar = c.p_start_next_bar = c.p_final_next_bar = buf;
    c.Rwb_bar_in = c.x_bar_in = c.xdot_bar_in = c.w_bar_in = c.joint_q_bar_in = buf;
    c.Rwb_bar = c.xdot_bar = c.w_bar = c.xdot_d_bar = c.joint_q_bar = c.p_start_bar = c.p_final_bar = buf;
    c.flags = words;
    CHECK(check_swing_reference_adjoint_args(h, 4097, &b, &c) == QC_OK, "every cotangent, every accumulator, every output");
  }
  {  // every cotangent alone, every output alone
    const double* qc_swing_reference_adjoint_io::* const cots[] = {&qc_swing_reference_adjoint_io::swing_pos_bar, &qc_swing_reference_adjoint_io::swing_vel_bar,
                                                                   &qc_swing_reference_adjoint_io::p_start_next_bar, &qc_swing_reference_adjoint_io::p_final_next_bar};
    double* qc_swing_reference_adjoint_io::* const outs[] = {&qc_swing_reference_adjoint_io::Rwb_bar,    &qc_swing_reference_adjoint_io::x_bar,
                                                             &qc_swing_reference_adjoint_io::xdot_bar,   &qc_swing_reference_adjoint_io::w_bar,
                                                             &qc_swing_reference_adjoint_io::xdot_d_bar, &qc_swing_reference_adjoint_io::joint_q_bar,
                                                             &qc_swing_reference_adjoint_io::p_start_bar, &qc_swing_reference_adjoint_io::p_final_bar};
    int k = 0;
    for (const auto m : cots) {
      qc_swing_reference_adjoint_io c{};
      c.struct_size = sizeof(qc_swing_reference_adjoint_io);
      c.state_before = records;
      c.*m = buf;
      c.flags = words;
      CHECK(check_swing_reference_adjoint_args(h, 1, &in, &c) == QC_OK, "cotangent %d alone, flags count as an output", k++);
    }
    k = 0;
    for (const auto m : outs) {
      qc_swing_reference_adjoint_io c{};
      c.struct_size = sizeof(qc_swing_reference_adjoint_io);
      c.state_before = records;
      c.p_final_next_bar = buf;
      c.*m = buf;
      CHECK(check_swing_reference_adjoint_args(h, 1, &in, &c) == QC_OK, "output %d alone", k++);
    }
  }
  const char* const null_arg = "qc_swing_reference_adjoint_batch: null argument";
  CHECK_FAILS(check_swing_reference_adjoint_args(nullptr, 1, &in, &io), null_arg, "no handle");
  CHECK_FAILS(check_swing_reference_adjoint_args(h, 1, nullptr, &io), null_arg, "no in");
  CHECK_FAILS(check_swing_reference_adjoint_args(h, 1, &in, nullptr), null_arg, "no io");
  for (const size_t sz : {(size_t)0, sizeof(qc_swing_reference_adjoint_io) - 8, sizeof(qc_swing_reference_adjoint_io) + 8, sizeof(qc_swing_reference_io)}) {
    qc_swing_reference_adjoint_io c = io;
    c.struct_size = sz;
    char text[360];
    std::snprintf(text, sizeof text,
                  "qc_swing_reference_adjoint_batch: qc_swing_reference_adjoint_io.struct_size is %zu, this library's qc_swing_reference_adjoint_io has %zu B "
                  "(qc_default_swing_reference_adjoint sets it)",
                  sz, sizeof(qc_swing_reference_adjoint_io));
    CHECK_FAILS(check_swing_reference_adjoint_args(h, 1, &in, &c), text, "struct_size %zu", sz);
    CHECK_FAILS(check_swing_reference_adjoint_args(h, 0, &in, &c), text, "struct_size %zu, n = 0", sz);
  }
  {
    const char* const text = "qc_swing_reference_adjoint_batch: swing_pos and swing_vel must be NULL (this call makes them)";
    qc_batch_in b = in;
    b.swing_vel = buf;
    CHECK_FAILS(check_swing_reference_adjoint_args(h, 1, &b, &io), text, "swing_vel given");
    CHECK_FAILS(check_swing_reference_adjoint_args(h, 0, &b, &io), text, "swing_vel given, n = 0");
  }
  {
    const char* const text = "qc_swing_reference_adjoint_batch: feet without joint_q (the planner starts from the forward kinematics of joint_q)";
    qc_batch_in b = in;
    b.joint_q = nullptr; b.feet = buf;
    CHECK_FAILS(check_swing_reference_adjoint_args(h, 1, &b, &io), text, "feet in place of joint_q");
  }
  {
    const char* const text =
        "qc_swing_reference_adjoint_batch: gait_dt must be NULL (the reverse pass advances no clock: gait_phase is read as the forward call left it)";
    qc_batch_in b = in;
    b.gait_dt = buf;
    CHECK_FAILS(check_swing_reference_adjoint_args(h, 1, &b, &io), text, "gait_dt");
    CHECK_FAILS(check_swing_reference_adjoint_args(h, 0, &b, &io), text, "gait_dt, n = 0");
  }
  {
    const char* const text = "qc_swing_reference_adjoint_batch: no cotangent given (swing_pos_bar, swing_vel_bar, p_start_next_bar, p_final_next_bar are all NULL)";
    qc_swing_reference_adjoint_io c = io;
    c.swing_pos_bar = nullptr;
    CHECK_FAILS(check_swing_reference_adjoint_args(h, 1, &in, &c), text, "no cotangent");
    CHECK_FAILS(check_swing_reference_adjoint_args(h, 0, &in, &c), text, "no cotangent, n = 0");
    c.Rwb_bar_in = c.x_bar_in = c.xdot_bar_in = c.w_bar_in = c.joint_q_bar_in = buf;
    CHECK_FAILS(check_swing_reference_adjoint_args(h, 1, &in, &c), text, "the accumulators are no cotangents");
  }
  {
    const char* const text =
        "qc_swing_reference_adjoint_batch: no output requested (Rwb_bar, x_bar, xdot_bar, w_bar, xdot_d_bar, joint_q_bar, p_start_bar, p_final_bar, flags are all NULL)";
    qc_swing_reference_adjoint_io c = io;
    c.x_bar = nullptr;
    CHECK_FAILS(check_swing_reference_adjoint_args(h, 1, &in, &c), text, "no output");
    CHECK_FAILS(check_swing_reference_adjoint_args(h, 0, &in, &c), text, "no output, n = 0");
  }
  {
    qc_swing_reference_adjoint_io c = io;
    c.state_before = nullptr;
    CHECK_FAILS(check_swing_reference_adjoint_args(h, 1, &in, &c), "qc_swing_reference_adjoint_batch: state_before is required (the swing records from before the forward call)",
                "no state_before");
    CHECK(check_swing_reference_adjoint_args(h, 0, &in, &c) == QC_OK, "no state_before, n = 0 asks for no array");
  }
  {
    const char* const text = "qc_swing_reference_adjoint_batch: Rwb, x, xdot, w, joint_q and gait_phase are required";
    const double* qc_batch_in::* const five[] = {&qc_batch_in::Rwb, &qc_batch_in::x, &qc_batch_in::xdot, &qc_batch_in::w, &qc_batch_in::joint_q};
    int k = 0;
    for (const auto m : five) {
      qc_batch_in b = in;
      b.*m = nullptr;
      CHECK_FAILS(check_swing_reference_adjoint_args(h, 1, &b, &io), text, "input %d missing", k);
      CHECK(check_swing_reference_adjoint_args(h, 0, &b, &io) == QC_OK, "input %d missing, n = 0 asks for no array", k);
      k++;
    }
    qc_batch_in b = in;
    b.gait_phase = nullptr;
    CHECK_FAILS(check_swing_reference_adjoint_args(h, 1, &b, &io), text, "no gait_phase");
  }
  const size_t most = (size_t)0xFFFFFF * SENSITIVITY_BLOCK;
  CHECK(check_swing_reference_adjoint_args(h, most, &in, &io) == QC_OK, "the largest batch of one launch");
  CHECK_FAILS(check_swing_reference_adjoint_args(h, most + 1, &in, &io), "qc_swing_reference_adjoint_batch: n is beyond one launch", "one robot more");
  CHECK(sizeof(qc_swing_reference_adjoint_io) == 20 * 8, "the io record: struct_size, state_before, four cotangents, five accumulators, nine outputs");
  CHECK(sizeof(qc_sensitivity_swing_io) == 13 * 8 && sizeof(qc_batch_in) == 18 * 8, "the neighbours keep their size");
}

int main() {
  forward();
  adjoint();
  std::printf("swing reference host logic ok (%ld checks)\n", g_checked);
  return 0;
}
