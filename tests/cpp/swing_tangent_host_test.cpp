// The device-free host logic of the swing legs' torque tangent (quadruped_control_amd/csrc/qc_host.hpp): check_swing_tangent_args
// through every refusal of qc_swing_torque_tangent_batch, swing_tangent_constants - the kernel's arguments -, swing_tangent_dirs and
// swing_tangent_blocks at, and one past, the grid cap.  Host compiler only - links neither HIP nor the library; built with the
// address and undefined-behaviour sanitizers (__graft_entry__.build_host_test) and run by tests/test_swing_tangent_cpu.py.  Prints
// the failing case and exits 1 on the first violated check.
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <string>

#include "host_check.hpp"

using namespace qc;

static double buf[32];
static int32_t ibuf[4];
static uint8_t bbuf[4];

static qc_batch_in valid_in() {
  qc_batch_in in{};
  in.Rwb = buf; in.x = buf + 1; in.joint_q = buf + 2; in.joint_qdot = buf + 3; in.swing_pos = buf + 4; in.swing_vel = buf + 5;
  return in;
}

static qc_swing_tangent_io valid_io() {
  qc_swing_tangent_io io{};
  io.struct_size = sizeof(qc_swing_tangent_io);
  io.n_dir = 1;
  io.joint_tau_tan_in = buf;
  io.joint_tau_tan = buf;  // over its input: the in-place chain behind qc_torque_tangent_batch
  return io;
}

static void arguments() {
  const qc_handle* const h = reinterpret_cast<const qc_handle*>(buf);  // only compared with null
  const qc_batch_in in = valid_in();
  const qc_swing_tangent_io io = valid_io();
  const char* const who = "qc_swing_torque_tangent_batch";
  const auto msg = [who](const char* what) { return std::string(who) + what; };
  CHECK(check_swing_tangent_args(h, 1, &in, &io) == QC_OK, "the smallest valid call (joint_tau_tan_in, written in place)");
  {
    qc_swing_tangent_io c = io;
    c.Rwb_rot_tan = buf + 6; c.x_tan = buf + 7; c.swing_pos_tan = buf + 8; c.swing_vel_tan = buf + 9; c.joint_q_tan = buf + 10; c.joint_qdot_tan = buf + 11;
    c.flags = ibuf;
    c.n_dir = 12;
    CHECK(check_swing_tangent_args(h, 4097, &in, &c) == QC_OK, "every tangent, both outputs, K = 12");
    c.joint_tau_tan = nullptr;
    CHECK(check_swing_tangent_args(h, 4097, &in, &c) == QC_OK, "the flags alone");
  }
  for (int k = 0; k < 7; k++) {  // each tangent alone
    qc_swing_tangent_io c = io;
    c.joint_tau_tan_in = nullptr;
    const double** const slot[7] = {&c.Rwb_rot_tan, &c.x_tan, &c.swing_pos_tan, &c.swing_vel_tan, &c.joint_q_tan, &c.joint_qdot_tan, &c.joint_tau_tan_in};
    *slot[k] = buf + 12;
    CHECK(check_swing_tangent_args(h, 1, &in, &c) == QC_OK, "tangent %d alone", k);
  }
  CHECK_FAILS(check_swing_tangent_args(nullptr, 1, &in, &io), msg(": null argument"), "no handle");
  CHECK_FAILS(check_swing_tangent_args(h, 1, nullptr, &io), msg(": null argument"), "no batch");
  CHECK_FAILS(check_swing_tangent_args(h, 1, &in, nullptr), msg(": null argument"), "no io");
  CHECK_FAILS(check_swing_tangent_args(nullptr, 0, &in, &io), msg(": null argument"), "no handle, n = 0");
  for (const size_t sz : {(size_t)0, sizeof(qc_swing_tangent_io) - 8, sizeof(qc_swing_tangent_io) + 8, sizeof(qc_torque_tangent_io)}) {
    qc_swing_tangent_io c = io;
    c.struct_size = sz;
    char text[320];
    std::snprintf(text, sizeof text, "%s: qc_swing_tangent_io.struct_size is %zu, this library's qc_swing_tangent_io has %zu B (qc_default_swing_tangent sets it)",
                  who, sz, sizeof(qc_swing_tangent_io));
    CHECK_FAILS(check_swing_tangent_args(h, 1, &in, &c), text, "struct_size %zu", sz);
    CHECK_FAILS(check_swing_tangent_args(h, 0, &in, &c), text, "struct_size %zu, n = 0", sz);
  }
  {
    qc_swing_tangent_io c = io;
    c.n_dir = 0;
    CHECK_FAILS(check_swing_tangent_args(h, 1, &in, &c), msg(": n_dir must be >= 1"), "n_dir 0");
    CHECK_FAILS(check_swing_tangent_args(h, 0, &in, &c), msg(": n_dir must be >= 1"), "n_dir 0, n = 0");
  }
  {
    const std::string none = msg(": no tangent given (Rwb_rot_tan, x_tan, swing_pos_tan, swing_vel_tan, joint_q_tan, joint_qdot_tan, joint_tau_tan_in are all NULL)");
    qc_swing_tangent_io c = io;
    c.joint_tau_tan_in = nullptr;
    CHECK_FAILS(check_swing_tangent_args(h, 1, &in, &c), none, "no tangent");
    CHECK_FAILS(check_swing_tangent_args(h, 0, &in, &c), none, "no tangent, n = 0");
  }
  {
    qc_swing_tangent_io c = io;
    c.joint_tau_tan = nullptr;
    CHECK_FAILS(check_swing_tangent_args(h, 1, &in, &c), msg(": no output requested (joint_tau_tan and flags are both NULL)"), "no output");
    CHECK_FAILS(check_swing_tangent_args(h, 0, &in, &c), msg(": no output requested (joint_tau_tan and flags are both NULL)"), "no output, n = 0");
  }
  {
    qc_batch_in c = in;
    c.swing_state = reinterpret_cast<qc_swing_state*>(buf);
    CHECK_FAILS(check_swing_tangent_args(h, 1, &c, &io),
                msg(": swing_state must be NULL (the planner's references have no forward mode: give swing_pos and swing_vel)"), "swing_state");
    CHECK_FAILS(check_swing_tangent_args(h, 0, &c, &io),
                msg(": swing_state must be NULL (the planner's references have no forward mode: give swing_pos and swing_vel)"), "swing_state, n = 0");
    c = in;
    c.gait_dt = buf;
    CHECK_FAILS(check_swing_tangent_args(h, 1, &c, &io), msg(": gait_dt must be NULL (the gait clock has no forward mode: the contact mask is read as it is now)"),
                "gait_dt");
  }
  for (int k = 0; k < 6; k++) {  // each of the six arrays missing
    qc_batch_in c = in;
    const double** const slot[6] = {&c.Rwb, &c.x, &c.joint_q, &c.joint_qdot, &c.swing_pos, &c.swing_vel};
    *slot[k] = nullptr;
    CHECK_FAILS(check_swing_tangent_args(h, 1, &c, &io), msg(": Rwb, x, joint_q, joint_qdot, swing_pos and swing_vel are required"), "array %d missing", k);
    CHECK(check_swing_tangent_args(h, 0, &c, &io) == QC_OK, "array %d missing, n = 0 asks for no array", k);
  }
  // one lane per (direction, robot, leg): the rows must fit a launch
  const size_t most = (size_t)0xFFFFFF * SWING_TANGENT_BLOCK / 4;
  CHECK(check_swing_tangent_args(h, most, &in, &io) == QC_OK, "the largest batch of one launch, K = 1");
  CHECK_FAILS(check_swing_tangent_args(h, most + 1, &in, &io), msg(": 4 * n * n_dir is beyond one launch"), "one robot more");
  {
    qc_swing_tangent_io c = io;
    c.n_dir = 16;
    CHECK(check_swing_tangent_args(h, (size_t)0xFFFFFF, &in, &c) == QC_OK, "the largest 4 n K, K = 16");
    CHECK_FAILS(check_swing_tangent_args(h, (size_t)0xFFFFFF + 1, &in, &c), msg(": 4 * n * n_dir is beyond one launch"), "one robot more at K = 16");
    c.n_dir = most;
    CHECK(check_swing_tangent_args(h, 1, &in, &c) == QC_OK, "one robot, the most directions");
    c.n_dir = most + 1;
    CHECK_FAILS(check_swing_tangent_args(h, 1, &in, &c), msg(": 4 * n * n_dir is beyond one launch"), "one direction more");
    c.n_dir = std::numeric_limits<size_t>::max();  // (a product that would wrap)
    CHECK_FAILS(check_swing_tangent_args(h, 3, &in, &c), msg(": 4 * n * n_dir is beyond one launch"), "n_dir = SIZE_MAX");
    CHECK_FAILS(check_swing_tangent_args(h, std::numeric_limits<size_t>::max() / 2, &in, &c), msg(": 4 * n * n_dir is beyond one launch"), "n and n_dir huge");
    CHECK(check_swing_tangent_args(h, 0, &in, &c) == QC_OK, "n = 0 launches nothing whatever n_dir is");
  }
  // the record: the layout the Python mirror restates
  CHECK(sizeof(qc_swing_tangent_io) == 11 * 8, "the io record: struct_size, n_dir, seven tangents, two outputs");
  CHECK(offsetof(qc_swing_tangent_io, n_dir) == 8 && offsetof(qc_swing_tangent_io, Rwb_rot_tan) == 16 && offsetof(qc_swing_tangent_io, x_tan) == 24 &&
            offsetof(qc_swing_tangent_io, swing_pos_tan) == 32 && offsetof(qc_swing_tangent_io, swing_vel_tan) == 40 &&
            offsetof(qc_swing_tangent_io, joint_q_tan) == 48 && offsetof(qc_swing_tangent_io, joint_qdot_tan) == 56 &&
            offsetof(qc_swing_tangent_io, joint_tau_tan_in) == 64 && offsetof(qc_swing_tangent_io, joint_tau_tan) == 72 && offsetof(qc_swing_tangent_io, flags) == 80,
        "the offsets of the record");
  CHECK(sizeof(qc_tangent_io) == 17 * 8 && sizeof(qc_plant_tangent_io) == 20 * 8 && sizeof(qc_torque_tangent_io) == 7 * 8, "the other records keep their sizes");
}

// what qc_default_swing_tangent leaves: the zeroed record with its size and one direction (the library's function is those three lines)
static void default_record() {
  qc_swing_tangent_io io{};
  io.struct_size = sizeof io;
  io.n_dir = 1;
  const qc_handle* const h = reinterpret_cast<const qc_handle*>(buf);
  const qc_batch_in in = valid_in();
  CHECK_FAILS(check_swing_tangent_args(h, 1, &in, &io),
              "qc_swing_torque_tangent_batch: no tangent given (Rwb_rot_tan, x_tan, swing_pos_tan, swing_vel_tan, joint_q_tan, joint_qdot_tan, joint_tau_tan_in are all NULL)",
              "the default record asks for nothing yet");
  io.x_tan = buf;
  io.flags = ibuf;
  CHECK(check_swing_tangent_args(h, 1, &in, &io) == QC_OK, "the default record with one tangent and one output");
}

static void constants() {
  qc_batch_in in = valid_in();
  in.stance = bbuf; in.gait_phase = buf + 13; in.gait_duty = buf + 14;
  in.feet = buf + 21; in.xdot = buf + 22;  // (not the kernel's business)
  qc_swing_tangent_io io{};
  io.n_dir = 7;
  io.Rwb_rot_tan = buf + 6; io.x_tan = buf + 7; io.swing_pos_tan = buf + 8; io.swing_vel_tan = buf + 9; io.joint_q_tan = buf + 10; io.joint_qdot_tan = buf + 11;
  io.joint_tau_tan_in = buf + 12; io.joint_tau_tan = buf + 15; io.flags = ibuf;
  SwingTangentArgs a = swing_tangent_constants(&in, &io);
  CHECK(a.Rwb == buf && a.x == buf + 1 && a.joint_q == buf + 2 && a.joint_qdot == buf + 3 && a.swing_pos == buf + 4 && a.swing_vel == buf + 5,
        "the six arrays of the batch");
  CHECK(a.stance == bbuf && a.gait_phase == buf + 13 && a.gait_duty == buf + 14, "the contact inputs of the batch");
  CHECK(a.n_dir == 7 && a.Rwb_rot_tan == buf + 6 && a.x_tan == buf + 7 && a.swing_pos_tan == buf + 8 && a.swing_vel_tan == buf + 9 && a.joint_q_tan == buf + 10 &&
            a.joint_qdot_tan == buf + 11 && a.joint_tau_tan_in == buf + 12 && a.joint_tau_tan == buf + 15 && a.flags == ibuf,
        "the record's arrays and K");
  CHECK(swing_tangent_dirs(&io) == 7, "every direction is walked for joint_tau_tan");
  io.joint_tau_tan = nullptr;
  a = swing_tangent_constants(&in, &io);
  CHECK(swing_tangent_dirs(&io) == 1 && a.n_dir == 1 && a.joint_tau_tan == nullptr && a.flags == ibuf, "the flags alone: one direction is walked");
  CHECK(sizeof(SwingTangentArgs) == 19 * 8, "the kernarg layout is the flat one");
}

static void blocks() {
  CHECK(swing_tangent_blocks(1, 1) == 1 && swing_tangent_blocks(16, 1) == 1 && swing_tangent_blocks(17, 1) == 2, "one wave of 16 robots' legs per workgroup");
  CHECK(swing_tangent_blocks(6, 3) == 2 && swing_tangent_blocks(16, 12) == 12, "K multiplies the rows");
  const size_t cap = (size_t)SWING_TANGENT_MAX_BLOCKS * SWING_TANGENT_BLOCK / 4;  // the robots of a full grid at K = 1
  CHECK(swing_tangent_blocks(cap, 1) == SWING_TANGENT_MAX_BLOCKS && swing_tangent_blocks(cap - 16, 1) == SWING_TANGENT_MAX_BLOCKS - 1, "at the cap, and one wave below it");
  CHECK(swing_tangent_blocks(cap + 1, 1) == SWING_TANGENT_MAX_BLOCKS && swing_tangent_blocks(cap / 4 + 1, 4) == SWING_TANGENT_MAX_BLOCKS,
        "one past the cap: the waves stride beyond it");
}

int main() {
  arguments();
  default_record();
  constants();
  blocks();
  std::printf("swing tangent host logic ok (%ld checks)\n", g_checked);
  return 0;
}
