// The device-free host logic of the forward-mode entry point (quadruped_control_amd/csrc/qc_host.hpp): check_tangent_args through
// every refusal of qc_tangent_batch and their order, tangent_constants, the grid the entry point launches and the [K][n] offset
// arithmetic.  Host compiler only - links neither HIP nor the library; built with the address and undefined-behaviour sanitizers
// (__graft_entry__.build_host_test) and run by tests/test_tangent_cpu.py.  Prints the failing case and exits 1 on the first
// violated check.
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
static qc_tangent_io valid_io() {
  qc_tangent_io io{};
  io.struct_size = sizeof(qc_tangent_io);
  io.grf_body = buf;
  io.act_tol = 1e-7;
  io.n_dir = 1;
  io.x_tan = buf;
  io.grf_tan = buf;
  return io;
}

static const double* qc_tangent_io::* const kTangents[] = {&qc_tangent_io::x_tan,      &qc_tangent_io::xdot_tan,    &qc_tangent_io::w_tan,
                                                           &qc_tangent_io::x_d_tan,    &qc_tangent_io::xdot_d_tan,  &qc_tangent_io::w_d_tan,
                                                           &qc_tangent_io::Rwb_rot_tan, &qc_tangent_io::Rwb_d_rot_tan, &qc_tangent_io::feet_tan};

static void arguments() {
  const qc_handle* const h = reinterpret_cast<const qc_handle*>(buf);  // only compared with null
  const qc_batch_in in = valid_in();
  const qc_tangent_io io = valid_io();
  CHECK(check_tangent_args(h, 1, &in, &io) == QC_OK, "the smallest valid call (one tangent, one output)");
  {
    qc_batch_in b = in;
    b.feet = nullptr; b.joint_q = buf; b.stance = bytes; b.gait_phase = buf; b.gait_duty = buf;
    b.gait_dt = buf; b.swing_pos = b.swing_vel = b.joint_qdot = buf;  // ignored, not refused
    qc_tangent_io c = io;
    for (const auto m : kTangents) c.*m = buf;
    c.joint_q_tan = buf; c.b_tan = buf; c.flags = &word; c.n_dir = 30;
    CHECK(check_tangent_args(h, 4097, &b, &c) == QC_OK, "joint_q, every tangent and every output, K = 30");
  }
  const char* const null_arg = "qc_tangent_batch: null argument";
  CHECK_FAILS(check_tangent_args(nullptr, 1, &in, &io), null_arg, "no handle");
  CHECK_FAILS(check_tangent_args(h, 1, nullptr, &io), null_arg, "no in");
  CHECK_FAILS(check_tangent_args(h, 1, &in, nullptr), null_arg, "no io");
  CHECK_FAILS(check_tangent_args(nullptr, 0, &in, &io), null_arg, "no handle, n = 0");
  for (const size_t sz : {(size_t)0, sizeof(qc_tangent_io) - 8, sizeof(qc_tangent_io) + 8, sizeof(qc_sensitivity_io)}) {
    qc_tangent_io c = io;
    c.struct_size = sz;
    c.act_tol = kNan;  // the record's size is judged before anything in it
    char text[224];
    std::snprintf(text, sizeof(text), "qc_tangent_batch: qc_tangent_io.struct_size is %zu, this library's qc_tangent_io has %zu B (qc_default_tangent sets it)", sz,
                  sizeof(qc_tangent_io));
    CHECK_FAILS(check_tangent_args(h, 1, &in, &c), text, "struct_size %zu", sz);
    CHECK_FAILS(check_tangent_args(h, 0, &in, &c), text, "struct_size %zu, n = 0", sz);
  }
  const char* const tol = "qc_tangent_batch: act_tol must be finite and >= 0";
  for (const double bad : {-1e-300, -1.0, kInf, -kInf, kNan}) {
    qc_tangent_io c = io;
    c.act_tol = bad;
    c.n_dir = 0;  // act_tol is judged before n_dir
    CHECK_FAILS(check_tangent_args(h, 1, &in, &c), tol, "act_tol = %g", bad);
    CHECK_FAILS(check_tangent_args(h, 0, &in, &c), tol, "act_tol = %g, n = 0", bad);
  }
  {
    qc_tangent_io c = io;
    c.act_tol = 0.0;
    CHECK(check_tangent_args(h, 1, &in, &c) == QC_OK, "a zero tolerance is allowed");
  }
  const char* const dirs = "qc_tangent_batch: n_dir must be >= 1";
  const char* const no_out = "qc_tangent_batch: no output requested (grf_tan and b_tan are both NULL)";
  const char* const no_tan =
      "qc_tangent_batch: no tangent given (x_tan, xdot_tan, w_tan, x_d_tan, xdot_d_tan, w_d_tan, Rwb_rot_tan, Rwb_d_rot_tan, feet_tan, joint_q_tan are all NULL)";
  const char* const jq = "qc_tangent_batch: joint_q_tan needs joint_q";
  const char* const forces = "qc_tangent_batch: grf_body is required";
  {
    qc_tangent_io c = io;
    c.n_dir = 0; c.grf_tan = nullptr;  // n_dir is judged before the outputs
    CHECK_FAILS(check_tangent_args(h, 1, &in, &c), dirs, "n_dir = 0");
    CHECK_FAILS(check_tangent_args(h, 0, &in, &c), dirs, "n_dir = 0, n = 0");
    c = io; c.grf_tan = nullptr; c.x_tan = nullptr;  // the outputs before the tangents
    CHECK_FAILS(check_tangent_args(h, 1, &in, &c), no_out, "no output");
    CHECK_FAILS(check_tangent_args(h, 0, &in, &c), no_out, "no output, n = 0");
    c = io; c.grf_tan = nullptr; c.flags = &word;
    CHECK_FAILS(check_tangent_args(h, 1, &in, &c), no_out, "flags alone are no output");
    c = io; c.grf_tan = nullptr; c.b_tan = buf;
    CHECK(check_tangent_args(h, 1, &in, &c) == QC_OK, "b_tan alone");
    c = io; c.x_tan = nullptr; c.grf_body = nullptr;  // the tangents before grf_body
    CHECK_FAILS(check_tangent_args(h, 1, &in, &c), no_tan, "no tangent");
    CHECK_FAILS(check_tangent_args(h, 0, &in, &c), no_tan, "no tangent, n = 0");
    for (size_t m = 0; m < sizeof(kTangents) / sizeof(kTangents[0]); m++) {
      c = io; c.x_tan = nullptr; c.*kTangents[m] = buf;
      CHECK(check_tangent_args(h, 1, &in, &c) == QC_OK, "tangent %zu alone", m);
    }
    c = io; c.joint_q_tan = buf; c.grf_body = nullptr;  // feet without joint_q; judged before grf_body
    CHECK_FAILS(check_tangent_args(h, 1, &in, &c), jq, "joint_q_tan on a batch with feet");
    CHECK_FAILS(check_tangent_args(h, 0, &in, &c), jq, "joint_q_tan on a batch with feet, n = 0");
    qc_batch_in b = in;
    b.joint_q = buf;
    c = io; c.x_tan = nullptr; c.joint_q_tan = buf;
    CHECK(check_tangent_args(h, 1, &b, &c) == QC_OK, "joint_q_tan alone on a batch with joint_q (feet given too)");
    c = io; c.grf_body = nullptr;
    b = in; b.Rwb = nullptr;  // grf_body before the state arrays
    CHECK_FAILS(check_tangent_args(h, 1, &b, &c), forces, "no grf_body");
    CHECK(check_tangent_args(h, 0, &b, &c) == QC_OK, "n = 0 asks for no array");
  }
  const char* const state = "qc_tangent_batch: the state arrays Rwb, Rwb_d, x, xdot, w, x_d, xdot_d and w_d are required (commander mode is out of scope)";
  const double* qc_batch_in::* const members[] = {&qc_batch_in::Rwb, &qc_batch_in::Rwb_d, &qc_batch_in::x, &qc_batch_in::xdot,
                                                  &qc_batch_in::w, &qc_batch_in::x_d, &qc_batch_in::xdot_d, &qc_batch_in::w_d};
  for (size_t m = 0; m < sizeof(members) / sizeof(members[0]); m++) {
    qc_batch_in b = in;
    b.*members[m] = nullptr;
    b.feet = nullptr;  // the state before the feet
    CHECK_FAILS(check_tangent_args(h, 1, &b, &io), state, "state array %zu missing", m);
    CHECK(check_tangent_args(h, 0, &b, &io) == QC_OK, "state array %zu missing, n = 0", m);
  }
  {
    qc_batch_in b = in;
    b.feet = nullptr;
    CHECK_FAILS(check_tangent_args(h, (size_t)0xFFFFFF * TANGENT_BLOCK + 1, &b, &io), "qc_tangent_batch: feet or joint_q is required",
                "neither feet nor joint_q (before the launch bound)");
    b.joint_q = buf;
    CHECK(check_tangent_args(h, 1, &b, &io) == QC_OK, "joint_q in place of feet");
  }
  const size_t most = (size_t)0xFFFFFF * TANGENT_BLOCK;
  CHECK(check_tangent_args(h, most, &in, &io) == QC_OK, "the largest batch of one launch");
  CHECK_FAILS(check_tangent_args(h, most + 1, &in, &io), "qc_tangent_batch: n is beyond one launch", "one robot more");
}

static void constants() {
  static double arr[13];
  qc_tangent_io io = valid_io();
  io.grf_body = arr; io.act_tol = 3e-5; io.n_dir = 7;
  io.x_tan = arr + 1; io.xdot_tan = arr + 2; io.w_tan = arr + 3; io.x_d_tan = arr + 4; io.xdot_d_tan = arr + 5; io.w_d_tan = arr + 6;
  io.Rwb_rot_tan = arr + 7; io.Rwb_d_rot_tan = arr + 8; io.feet_tan = arr + 9; io.joint_q_tan = arr + 10;
  io.grf_tan = arr + 11; io.b_tan = arr + 12; io.flags = &word;
  const TangentArgs a = tangent_constants(&io);
  CHECK(a.grf_body == arr && a.act_tol == 3e-5 && a.n_dir == 7, "the forces and the scalars");
  CHECK(a.x_tan == arr + 1 && a.xdot_tan == arr + 2 && a.w_tan == arr + 3 && a.x_d_tan == arr + 4 && a.xdot_d_tan == arr + 5 && a.w_d_tan == arr + 6 &&
            a.Rwb_rot_tan == arr + 7 && a.Rwb_d_rot_tan == arr + 8 && a.feet_tan == arr + 9 && a.joint_q_tan == arr + 10,
        "every tangent lands in its own field");
  CHECK(a.grf_tan == arr + 11 && a.b_tan == arr + 12 && a.flags == &word, "the outputs");
  CHECK(sizeof(qc_tangent_io) == 17 * 8, "the io record: struct_size, grf_body, act_tol, n_dir, ten tangents and three outputs");
}

static void grid_and_offsets() {
  CHECK(tangent_blocks(1) == 1 && tangent_blocks(64) == 1 && tangent_blocks(65) == 2 && tangent_blocks(130) == 3 && tangent_blocks(1000) == 16,
        "one wave per 64 robots");
  const size_t cap = (size_t)TANGENT_MAX_BLOCKS * TANGENT_BLOCK;
  CHECK(tangent_blocks(cap) == (unsigned)TANGENT_MAX_BLOCKS && tangent_blocks(cap + 1) == (unsigned)TANGENT_MAX_BLOCKS &&
            tangent_blocks(262209) == (unsigned)TANGENT_MAX_BLOCKS && tangent_blocks((size_t)0xFFFFFF * TANGENT_BLOCK) == (unsigned)TANGENT_MAX_BLOCKS,
        "the grid is capped: the waves stride beyond it");
  // direction k of an [n][m] array starts at ptr + k n m: robot i of direction k is row k n + i
  CHECK(tangent_row(0, 65, 0) == 0 && tangent_row(0, 65, 64) == 64, "n_dir = 1: the rows of an [n][m] array");
  CHECK(tangent_row(1, 65, 0) == 65 && tangent_row(2, 65, 64) == 194 && 3 * tangent_row(2, 65, 64) + 2 == 3 * 3 * 65 - 1,
        "n_dir = 3: the last value of an [3][65][3] array is the last of direction 2");
  CHECK(4 * tangent_row(2, 65, 64) + 3 == 3 * 65 * 4 - 1 && 2 * tangent_row(2, 65, 64) + 1 == 3 * 65 * 2 - 1, "the last foot of grf_tan and the last half of b_tan");
  CHECK(tangent_row(29, 262209, 262208) == 30L * 262209 - 1 && 12 * tangent_row(29, 16777215L * 64, 0) > (1L << 32), "no 32-bit arithmetic");
}

int main() {
  arguments();
  constants();
  grid_and_offsets();
  std::printf("tangent host logic ok (%ld checks)\n", g_checked);
  return 0;
}
