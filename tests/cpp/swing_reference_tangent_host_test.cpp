// The device-free host logic of the swing references' forward mode (quadruped_control_amd/csrc/qc_host.hpp):
// check_swing_reference_tangent_args through every refusal of qc_swing_reference_tangent_batch, swing_reference_tangent_constants - the
// kernel's arguments -, swing_reference_tangent_dirs and swing_reference_tangent_blocks at, and one past, the grid cap.  Host compiler
// only - links neither HIP nor the library; built with the address and undefined-behaviour sanitizers
// (__graft_entry__.build_host_test) and run by tests/test_swing_reference_tangent_cpu.py.  Prints the failing case and exits 1 on the
// first violated check.
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <string>

#include "host_check.hpp"

using namespace qc;

static double buf[40];
static int32_t ibuf[4];
static uint8_t bbuf[4];
static qc_swing_state records[1];

static qc_batch_in valid_in() {
  qc_batch_in in{};
  in.Rwb = buf; in.x = buf + 1; in.xdot = buf + 2; in.w = buf + 3; in.joint_q = buf + 4; in.gait_phase = buf + 5;
  return in;
}

static qc_swing_reference_tangent_io valid_io() {
  qc_swing_reference_tangent_io io{};
  io.struct_size = sizeof(qc_swing_reference_tangent_io);
  io.state_before = records;
  io.n_dir = 1;
  io.p_start_tan = buf + 6;
  io.p_start_next_tan = buf + 6;  // over its input: a rollout carries the record's tangents in place
  return io;
}

static void arguments() {
  const qc_handle* const h = reinterpret_cast<const qc_handle*>(buf);  // only compared with null
  const qc_batch_in in = valid_in();
  const qc_swing_reference_tangent_io io = valid_io();
  const char* const who = "qc_swing_reference_tangent_batch";
  const auto msg = [who](const char* what) { return std::string(who) + what; };
  CHECK(check_swing_reference_tangent_args(h, 1, &in, &io) == QC_OK, "the smallest valid call (p_start_tan, written in place)");
  {
    qc_swing_reference_tangent_io c = io;
    c.Rwb_rot_tan = buf + 7; c.x_tan = buf + 8; c.xdot_tan = buf + 9; c.w_tan = buf + 10; c.xdot_d_tan = buf + 11; c.joint_q_tan = buf + 12;
    c.p_final_tan = buf + 13; c.p_final_next_tan = buf + 13; c.swing_pos_tan = buf + 14; c.swing_vel_tan = buf + 15; c.flags = ibuf;
    c.n_dir = 12;
    qc_batch_in b = in;
    b.stance = bbuf; b.gait_duty = buf + 16; b.xdot_d = buf + 17; b.swing_state = records;  // optional, or not this call's business
    CHECK(check_swing_reference_tangent_args(h, 4097, &b, &c) == QC_OK, "every tangent, every output, K = 12");
    c.swing_pos_tan = c.swing_vel_tan = c.p_start_next_tan = c.p_final_next_tan = nullptr;
    CHECK(check_swing_reference_tangent_args(h, 4097, &b, &c) == QC_OK, "the flags alone");
  }
  for (int k = 0; k < 8; k++) {  // each tangent alone
    qc_swing_reference_tangent_io c = io;
    c.p_start_tan = nullptr;
    const double** const slot[8] = {&c.Rwb_rot_tan, &c.x_tan, &c.xdot_tan, &c.w_tan, &c.xdot_d_tan, &c.joint_q_tan, &c.p_start_tan, &c.p_final_tan};
    *slot[k] = buf + 18;
    CHECK(check_swing_reference_tangent_args(h, 1, &in, &c) == QC_OK, "tangent %d alone", k);
  }
  for (int k = 0; k < 5; k++) {  // each output alone
    qc_swing_reference_tangent_io c = io;
    c.p_start_next_tan = nullptr;
    if (k == 4) c.flags = ibuf;
    else {
      double** const slot[4] = {&c.swing_pos_tan, &c.swing_vel_tan, &c.p_start_next_tan, &c.p_final_next_tan};
      *slot[k] = buf + 19;
    }
    CHECK(check_swing_reference_tangent_args(h, 1, &in, &c) == QC_OK, "output %d alone", k);
  }
  CHECK_FAILS(check_swing_reference_tangent_args(nullptr, 1, &in, &io), msg(": null argument"), "no handle");
  CHECK_FAILS(check_swing_reference_tangent_args(h, 1, nullptr, &io), msg(": null argument"), "no batch");
  CHECK_FAILS(check_swing_reference_tangent_args(h, 1, &in, nullptr), msg(": null argument"), "no io");
  CHECK_FAILS(check_swing_reference_tangent_args(nullptr, 0, &in, &io), msg(": null argument"), "no handle, n = 0");
  for (const size_t sz : {(size_t)0, sizeof(qc_swing_reference_tangent_io) - 8, sizeof(qc_swing_reference_tangent_io) + 8, sizeof(qc_swing_tangent_io)}) {
    qc_swing_reference_tangent_io c = io;
    c.struct_size = sz;
    char text[360];
    std::snprintf(text, sizeof text,
                  "%s: qc_swing_reference_tangent_io.struct_size is %zu, this library's qc_swing_reference_tangent_io has %zu B (qc_default_swing_reference_tangent sets it)",
                  who, sz, sizeof(qc_swing_reference_tangent_io));
    CHECK_FAILS(check_swing_reference_tangent_args(h, 1, &in, &c), text, "struct_size %zu", sz);
    CHECK_FAILS(check_swing_reference_tangent_args(h, 0, &in, &c), text, "struct_size %zu, n = 0", sz);
  }
  {
    qc_swing_reference_tangent_io c = io;
    c.n_dir = 0;
    CHECK_FAILS(check_swing_reference_tangent_args(h, 1, &in, &c), msg(": n_dir must be >= 1"), "n_dir 0");
    CHECK_FAILS(check_swing_reference_tangent_args(h, 0, &in, &c), msg(": n_dir must be >= 1"), "n_dir 0, n = 0");
  }
  {
    const std::string none = msg(": no tangent given (Rwb_rot_tan, x_tan, xdot_tan, w_tan, xdot_d_tan, joint_q_tan, p_start_tan, p_final_tan are all NULL)");
    qc_swing_reference_tangent_io c = io;
    c.p_start_tan = nullptr;
    CHECK_FAILS(check_swing_reference_tangent_args(h, 1, &in, &c), none, "no tangent");
    CHECK_FAILS(check_swing_reference_tangent_args(h, 0, &in, &c), none, "no tangent, n = 0");
  }
  {
    const std::string none = msg(": no output requested (swing_pos_tan, swing_vel_tan, p_start_next_tan, p_final_next_tan, flags are all NULL)");
    qc_swing_reference_tangent_io c = io;
    c.p_start_next_tan = nullptr;
    CHECK_FAILS(check_swing_reference_tangent_args(h, 1, &in, &c), none, "no output");
    CHECK_FAILS(check_swing_reference_tangent_args(h, 0, &in, &c), none, "no output, n = 0");
  }
  {
    qc_batch_in c = in;
    c.gait_dt = buf;
    const std::string clock = msg(": gait_dt must be NULL (no clock is advanced here: gait_phase is read as the forward call left it)");
    CHECK_FAILS(check_swing_reference_tangent_args(h, 1, &c, &io), clock, "gait_dt");
    CHECK_FAILS(check_swing_reference_tangent_args(h, 0, &c, &io), clock, "gait_dt, n = 0");
    const std::string refs = msg(": swing_pos and swing_vel must be NULL (this call makes them)");
    c = in;
    c.swing_pos = buf;
    CHECK_FAILS(check_swing_reference_tangent_args(h, 1, &c, &io), refs, "swing_pos");
    c = in;
    c.swing_vel = buf;
    CHECK_FAILS(check_swing_reference_tangent_args(h, 1, &c, &io), refs, "swing_vel");
    c = in;
    c.feet = buf;
    c.joint_q = nullptr;
    CHECK_FAILS(check_swing_reference_tangent_args(h, 1, &c, &io), msg(": feet without joint_q (the planner starts from the forward kinematics of joint_q)"),
                "feet without joint_q");
    c.joint_q = buf + 4;
    CHECK(check_swing_reference_tangent_args(h, 1, &c, &io) == QC_OK, "feet beside joint_q are ignored");
  }
  {
    qc_swing_reference_tangent_io c = io;
    c.state_before = nullptr;
    CHECK_FAILS(check_swing_reference_tangent_args(h, 1, &in, &c), msg(": state_before is required (the swing records from before the forward call)"), "no state_before");
    CHECK(check_swing_reference_tangent_args(h, 0, &in, &c) == QC_OK, "no state_before, n = 0 asks for no array");
  }
  for (int k = 0; k < 6; k++) {  // each of the six arrays missing
    qc_batch_in c = in;
    const double** const slot[5] = {&c.Rwb, &c.x, &c.xdot, &c.w, &c.joint_q};
    if (k < 5) *slot[k] = nullptr;
    else c.gait_phase = nullptr;
    CHECK_FAILS(check_swing_reference_tangent_args(h, 1, &c, &io), msg(": Rwb, x, xdot, w, joint_q and gait_phase are required"), "array %d missing", k);
    CHECK(check_swing_reference_tangent_args(h, 0, &c, &io) == QC_OK, "array %d missing, n = 0 asks for no array", k);
  }
  // one lane per (direction, robot): the pairs must fit a launch
  const size_t most = (size_t)0xFFFFFF * SWING_REFERENCE_TANGENT_BLOCK;
  CHECK(check_swing_reference_tangent_args(h, most, &in, &io) == QC_OK, "the largest batch of one launch, K = 1");
  CHECK_FAILS(check_swing_reference_tangent_args(h, most + 1, &in, &io), msg(": n * n_dir is beyond one launch"), "one robot more");
  {
    qc_swing_reference_tangent_io c = io;
    c.n_dir = 64;
    CHECK(check_swing_reference_tangent_args(h, (size_t)0xFFFFFF, &in, &c) == QC_OK, "the largest n K, K = 64");
    CHECK_FAILS(check_swing_reference_tangent_args(h, (size_t)0xFFFFFF + 1, &in, &c), msg(": n * n_dir is beyond one launch"), "one robot more at K = 64");
    c.n_dir = most;
    CHECK(check_swing_reference_tangent_args(h, 1, &in, &c) == QC_OK, "one robot, the most directions");
    c.n_dir = most + 1;
    CHECK_FAILS(check_swing_reference_tangent_args(h, 1, &in, &c), msg(": n * n_dir is beyond one launch"), "one direction more");
    c.n_dir = std::numeric_limits<size_t>::max();  // (a product that would wrap)
    CHECK_FAILS(check_swing_reference_tangent_args(h, 3, &in, &c), msg(": n * n_dir is beyond one launch"), "n_dir = SIZE_MAX");
    CHECK_FAILS(check_swing_reference_tangent_args(h, std::numeric_limits<size_t>::max() / 2, &in, &c), msg(": n * n_dir is beyond one launch"), "n and n_dir huge");
    CHECK(check_swing_reference_tangent_args(h, 0, &in, &c) == QC_OK, "n = 0 launches nothing whatever n_dir is");
  }
  // the record: the layout the Python mirror restates
  CHECK(sizeof(qc_swing_reference_tangent_io) == 16 * 8, "the io record: struct_size, state_before, n_dir, eight tangents, five outputs");
  CHECK(offsetof(qc_swing_reference_tangent_io, state_before) == 8 && offsetof(qc_swing_reference_tangent_io, n_dir) == 16 &&
            offsetof(qc_swing_reference_tangent_io, Rwb_rot_tan) == 24 && offsetof(qc_swing_reference_tangent_io, x_tan) == 32 &&
            offsetof(qc_swing_reference_tangent_io, xdot_tan) == 40 && offsetof(qc_swing_reference_tangent_io, w_tan) == 48 &&
            offsetof(qc_swing_reference_tangent_io, xdot_d_tan) == 56 && offsetof(qc_swing_reference_tangent_io, joint_q_tan) == 64 &&
            offsetof(qc_swing_reference_tangent_io, p_start_tan) == 72 && offsetof(qc_swing_reference_tangent_io, p_final_tan) == 80 &&
            offsetof(qc_swing_reference_tangent_io, swing_pos_tan) == 88 && offsetof(qc_swing_reference_tangent_io, swing_vel_tan) == 96 &&
            offsetof(qc_swing_reference_tangent_io, p_start_next_tan) == 104 && offsetof(qc_swing_reference_tangent_io, p_final_next_tan) == 112 &&
            offsetof(qc_swing_reference_tangent_io, flags) == 120,
        "the offsets of the record");
  CHECK(sizeof(qc_tangent_io) == 17 * 8 && sizeof(qc_plant_tangent_io) == 20 * 8 && sizeof(qc_torque_tangent_io) == 7 * 8 && sizeof(qc_swing_tangent_io) == 11 * 8,
        "the other records keep their sizes");
}

// what qc_default_swing_reference_tangent leaves: the zeroed record with its size and one direction (the library's function is those three lines)
static void default_record() {
  qc_swing_reference_tangent_io io{};
  io.struct_size = sizeof io;
  io.n_dir = 1;
  const qc_handle* const h = reinterpret_cast<const qc_handle*>(buf);
  const qc_batch_in in = valid_in();
  CHECK_FAILS(check_swing_reference_tangent_args(h, 1, &in, &io),
              "qc_swing_reference_tangent_batch: no tangent given (Rwb_rot_tan, x_tan, xdot_tan, w_tan, xdot_d_tan, joint_q_tan, p_start_tan, p_final_tan are all NULL)",
              "the default record asks for nothing yet");
  io.x_tan = buf;
  io.flags = ibuf;
  io.state_before = records;
  CHECK(check_swing_reference_tangent_args(h, 1, &in, &io) == QC_OK, "the default record with one tangent, one output and the records");
}

static void constants() {
  qc_batch_in in = valid_in();
  in.stance = bbuf; in.gait_duty = buf + 20;
  in.xdot_d = buf + 21; in.joint_qdot = buf + 22;  // (not the kernel's business)
  qc_swing_reference_tangent_io io{};
  io.state_before = records;
  io.n_dir = 7;
  io.Rwb_rot_tan = buf + 7; io.x_tan = buf + 8; io.xdot_tan = buf + 9; io.w_tan = buf + 10; io.xdot_d_tan = buf + 11; io.joint_q_tan = buf + 12;
  io.p_start_tan = buf + 13; io.p_final_tan = buf + 14; io.swing_pos_tan = buf + 15; io.swing_vel_tan = buf + 16; io.p_start_next_tan = buf + 17;
  io.p_final_next_tan = buf + 18; io.flags = ibuf;
  SwingReferenceTangentArgs a = swing_reference_tangent_constants(&in, &io);
  CHECK(a.Rwb == buf && a.x == buf + 1 && a.xdot == buf + 2 && a.w == buf + 3 && a.joint_q == buf + 4 && a.gait_phase == buf + 5, "the six arrays of the batch");
  CHECK(a.stance == bbuf && a.gait_duty == buf + 20 && (const void*)a.before == (const void*)records, "the contact inputs of the batch and the records before the call");
  CHECK(a.n_dir == 7 && a.Rwb_rot_tan == buf + 7 && a.x_tan == buf + 8 && a.xdot_tan == buf + 9 && a.w_tan == buf + 10 && a.xdot_d_tan == buf + 11 &&
            a.joint_q_tan == buf + 12 && a.p_start_tan == buf + 13 && a.p_final_tan == buf + 14,
        "the record's tangents and K");
  CHECK(a.swing_pos_tan == buf + 15 && a.swing_vel_tan == buf + 16 && a.p_start_next_tan == buf + 17 && a.p_final_next_tan == buf + 18 && a.flags == ibuf,
        "the record's outputs");
  CHECK(swing_reference_tangent_dirs(&io) == 7, "every direction is walked for a row output");
  io.swing_pos_tan = io.swing_vel_tan = io.p_start_next_tan = nullptr;
  CHECK(swing_reference_tangent_dirs(&io) == 7, "one row output is enough");
  io.p_final_next_tan = nullptr;
  a = swing_reference_tangent_constants(&in, &io);
  CHECK(swing_reference_tangent_dirs(&io) == 1 && a.n_dir == 1 && a.flags == ibuf, "the flags alone: one direction is walked");
  CHECK(sizeof(SwingReferenceTangentArgs) == 23 * 8, "the kernarg layout is the flat one");
  CHECK(sizeof(SwingState) == sizeof(qc_swing_state), "the device's record is the header's");
}

static void blocks() {
  CHECK(swing_reference_tangent_blocks(1, 1) == 1 && swing_reference_tangent_blocks(64, 1) == 1 && swing_reference_tangent_blocks(65, 1) == 2,
        "one wave of 64 pairs per workgroup");
  CHECK(swing_reference_tangent_blocks(22, 3) == 2 && swing_reference_tangent_blocks(64, 12) == 12, "K multiplies the pairs");
  const size_t cap = (size_t)SWING_REFERENCE_TANGENT_MAX_BLOCKS * SWING_REFERENCE_TANGENT_BLOCK;  // the pairs of a full grid
  CHECK(swing_reference_tangent_blocks(cap, 1) == SWING_REFERENCE_TANGENT_MAX_BLOCKS &&
            swing_reference_tangent_blocks(cap - 64, 1) == SWING_REFERENCE_TANGENT_MAX_BLOCKS - 1,
        "at the cap, and one wave below it");
  CHECK(swing_reference_tangent_blocks(cap + 1, 1) == SWING_REFERENCE_TANGENT_MAX_BLOCKS &&
            swing_reference_tangent_blocks(cap / 4 + 1, 4) == SWING_REFERENCE_TANGENT_MAX_BLOCKS,
        "one past the cap: the waves stride beyond it");
}

int main() {
  arguments();
  default_record();
  constants();
  blocks();
  std::printf("swing reference tangent host logic ok (%ld checks)\n", g_checked);
  return 0;
}
