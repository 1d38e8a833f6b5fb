// The device-free host logic of the forward mode in the parameters (quadruped_control_amd/csrc/qc_host.hpp): check_param_tangent_args
// through every refusal of qc_param_tangent_batch and their order, param_tangent_constants, the grid the entry point launches and
// the offsets of a row of param_tan.  Host compiler only - links neither HIP nor the library; built with the address and
// undefined-behaviour sanitizers (__graft_entry__.build_host_test) and run by tests/test_param_tangent_cpu.py.  Prints the failing
// case and exits 1 on the first violated check.
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
static qc_param_tangent_io valid_io() {
  qc_param_tangent_io io{};
  io.struct_size = sizeof(qc_param_tangent_io);
  io.grf_body = buf;
  io.act_tol = 1e-7;
  io.n_dir = 1;
  io.param_tan = buf;
  io.grf_tan = buf;
  return io;
}

static void arguments() {
  const qc_handle* const h = reinterpret_cast<const qc_handle*>(buf);  // only compared with null
  const qc_batch_in in = valid_in();
  const qc_param_tangent_io io = valid_io();
  CHECK(check_param_tangent_args(h, 1, &in, &io) == QC_OK, "the smallest valid call (one direction, one output)");
  {
    qc_batch_in b = in;
    b.feet = nullptr; b.joint_q = buf; b.stance = bytes; b.gait_phase = buf; b.gait_duty = buf;
    b.gait_dt = buf; b.swing_pos = b.swing_vel = b.joint_qdot = buf;  // ignored, not refused
    qc_param_tangent_io c = io;
    c.grf_tan_in = buf; c.b_tan = buf; c.b_tan_in = buf; c.flags = &word; c.n_dir = 211;
    CHECK(check_param_tangent_args(h, 4097, &b, &c) == QC_OK, "joint_q, both outputs accumulated in place, K = 211");
  }
  const char* const null_arg = "qc_param_tangent_batch: null argument";
  CHECK_FAILS(check_param_tangent_args(nullptr, 1, &in, &io), null_arg, "no handle");
  CHECK_FAILS(check_param_tangent_args(h, 1, nullptr, &io), null_arg, "no in");
  CHECK_FAILS(check_param_tangent_args(h, 1, &in, nullptr), null_arg, "no io");
  CHECK_FAILS(check_param_tangent_args(nullptr, 0, &in, &io), null_arg, "no handle, n = 0");
  for (const size_t sz : {(size_t)0, sizeof(qc_param_tangent_io) - 8, sizeof(qc_param_tangent_io) + 8, sizeof(qc_tangent_io)}) {
    qc_param_tangent_io c = io;
    c.struct_size = sz;
    c.act_tol = kNan;  // the record's size is judged before anything in it
    char text[256];
    std::snprintf(text, sizeof(text),
                  "qc_param_tangent_batch: qc_param_tangent_io.struct_size is %zu, this library's qc_param_tangent_io has %zu B (qc_default_param_tangent sets it)",
                  sz, sizeof(qc_param_tangent_io));
    CHECK_FAILS(check_param_tangent_args(h, 1, &in, &c), text, "struct_size %zu", sz);
    CHECK_FAILS(check_param_tangent_args(h, 0, &in, &c), text, "struct_size %zu, n = 0", sz);
  }
  const char* const tol = "qc_param_tangent_batch: act_tol must be finite and >= 0";
  for (const double bad : {-1e-300, -1.0, kInf, -kInf, kNan}) {
    qc_param_tangent_io c = io;
    c.act_tol = bad;
    c.n_dir = 0;  // act_tol is judged before n_dir
    CHECK_FAILS(check_param_tangent_args(h, 1, &in, &c), tol, "act_tol = %g", bad);
    CHECK_FAILS(check_param_tangent_args(h, 0, &in, &c), tol, "act_tol = %g, n = 0", bad);
  }
  {
    qc_param_tangent_io c = io;
    c.act_tol = 0.0;
    CHECK(check_param_tangent_args(h, 1, &in, &c) == QC_OK, "a zero tolerance is allowed");
  }
  const char* const dirs = "qc_param_tangent_batch: n_dir must be >= 1";
  const char* const no_tan = "qc_param_tangent_batch: param_tan is required";
  const char* const no_out = "qc_param_tangent_batch: no output requested (grf_tan and b_tan are both NULL)";
  const char* const g_in = "qc_param_tangent_batch: grf_tan_in needs grf_tan";
  const char* const b_in = "qc_param_tangent_batch: b_tan_in needs b_tan";
  const char* const forces = "qc_param_tangent_batch: grf_body is required";
  {
    qc_param_tangent_io c = io;
    c.n_dir = 0; c.param_tan = nullptr;  // n_dir is judged before param_tan
    CHECK_FAILS(check_param_tangent_args(h, 1, &in, &c), dirs, "n_dir = 0");
    CHECK_FAILS(check_param_tangent_args(h, 0, &in, &c), dirs, "n_dir = 0, n = 0");
    c = io; c.param_tan = nullptr; c.grf_tan = nullptr;  // param_tan before the outputs
    CHECK_FAILS(check_param_tangent_args(h, 1, &in, &c), no_tan, "no param_tan");
    CHECK_FAILS(check_param_tangent_args(h, 0, &in, &c), no_tan, "no param_tan, n = 0");
    c = io; c.grf_tan = nullptr; c.b_tan_in = buf;  // the outputs before what is added to them
    CHECK_FAILS(check_param_tangent_args(h, 1, &in, &c), no_out, "no output");
    CHECK_FAILS(check_param_tangent_args(h, 0, &in, &c), no_out, "no output, n = 0");
    c = io; c.grf_tan = nullptr; c.flags = &word;
    CHECK_FAILS(check_param_tangent_args(h, 1, &in, &c), no_out, "flags alone are no output");
    c = io; c.grf_tan = nullptr; c.b_tan = buf;
    CHECK(check_param_tangent_args(h, 1, &in, &c) == QC_OK, "b_tan alone");
    c = io; c.grf_tan = nullptr; c.b_tan = buf; c.grf_tan_in = buf; c.b_tan_in = buf;
    CHECK_FAILS(check_param_tangent_args(h, 1, &in, &c), g_in, "grf_tan_in without grf_tan");
    c = io; c.b_tan_in = buf; c.grf_body = nullptr;  // judged before grf_body
    CHECK_FAILS(check_param_tangent_args(h, 1, &in, &c), b_in, "b_tan_in without b_tan");
    CHECK_FAILS(check_param_tangent_args(h, 0, &in, &c), b_in, "b_tan_in without b_tan, n = 0");
    c = io; c.grf_tan_in = buf;
    CHECK(check_param_tangent_args(h, 1, &in, &c) == QC_OK, "grf_tan_in IS grf_tan");
    c = io; c.grf_body = nullptr;
    qc_batch_in b = in;
    b.Rwb = nullptr;  // grf_body before the state arrays
    CHECK_FAILS(check_param_tangent_args(h, 1, &b, &c), forces, "no grf_body");
    CHECK(check_param_tangent_args(h, 0, &b, &c) == QC_OK, "n = 0 asks for no array");
  }
  const char* const state =
      "qc_param_tangent_batch: the state arrays Rwb, Rwb_d, x, xdot, w, x_d, xdot_d and w_d are required (commander mode is out of scope)";
  const double* qc_batch_in::* const members[] = {&qc_batch_in::Rwb, &qc_batch_in::Rwb_d, &qc_batch_in::x, &qc_batch_in::xdot,
                                                  &qc_batch_in::w, &qc_batch_in::x_d, &qc_batch_in::xdot_d, &qc_batch_in::w_d};
  for (size_t m = 0; m < sizeof(members) / sizeof(members[0]); m++) {
    qc_batch_in b = in;
    b.*members[m] = nullptr;
    b.feet = nullptr;  // the state before the feet
    CHECK_FAILS(check_param_tangent_args(h, 1, &b, &io), state, "state array %zu missing", m);
    CHECK(check_param_tangent_args(h, 0, &b, &io) == QC_OK, "state array %zu missing, n = 0", m);
  }
  {
    qc_batch_in b = in;
    b.feet = nullptr;
    CHECK_FAILS(check_param_tangent_args(h, (size_t)0xFFFFFF * PARAM_TANGENT_BLOCK + 1, &b, &io), "qc_param_tangent_batch: feet or joint_q is required",
                "neither feet nor joint_q (before the launch bound)");
    b.joint_q = buf;
    CHECK(check_param_tangent_args(h, 1, &b, &io) == QC_OK, "joint_q in place of feet");
  }
  const size_t most = (size_t)0xFFFFFF * PARAM_TANGENT_BLOCK;
  qc_param_tangent_io many = io;
  many.n_dir = 1000;  // one lane per robot whatever K is
  CHECK(check_param_tangent_args(h, most, &in, &many) == QC_OK, "the largest batch of one launch, K = 1000");
  CHECK_FAILS(check_param_tangent_args(h, most + 1, &in, &io), "qc_param_tangent_batch: n is beyond one launch", "one robot more");
}

static void constants() {
  static double arr[6];
  qc_param_tangent_io io = valid_io();
  io.grf_body = arr; io.act_tol = 3e-5; io.n_dir = 7;
  io.param_tan = arr + 1; io.grf_tan_in = arr + 2; io.b_tan_in = arr + 3; io.grf_tan = arr + 4; io.b_tan = arr + 5; io.flags = &word;
  const ParamTangentArgs a = param_tangent_constants(&io);
  CHECK(a.grf_body == arr && a.act_tol == 3e-5 && a.n_dir == 7, "the forces and the scalars");
  CHECK(a.param_tan == arr + 1 && a.grf_tan_in == arr + 2 && a.b_tan_in == arr + 3, "the directions and what is added land in their own fields");
  CHECK(a.grf_tan == arr + 4 && a.b_tan == arr + 5 && a.flags == &word, "the outputs");
  CHECK(sizeof(qc_param_tangent_io) == 10 * 8, "the io record: struct_size, grf_body, act_tol, n_dir, param_tan, two added arrays and three outputs");
}

static void grid_and_layout() {
  CHECK(param_tangent_blocks(1) == 1 && param_tangent_blocks(64) == 1 && param_tangent_blocks(65) == 2 && param_tangent_blocks(130) == 3 &&
            param_tangent_blocks(1000) == 16,
        "one wave per 64 robots");
  const size_t cap = (size_t)PARAM_TANGENT_MAX_BLOCKS * PARAM_TANGENT_BLOCK;
  CHECK(param_tangent_blocks(cap) == (unsigned)PARAM_TANGENT_MAX_BLOCKS && param_tangent_blocks(cap + 1) == (unsigned)PARAM_TANGENT_MAX_BLOCKS &&
            param_tangent_blocks((size_t)0xFFFFFF * PARAM_TANGENT_BLOCK) == (unsigned)PARAM_TANGENT_MAX_BLOCKS,
        "the grid is capped: the waves stride beyond it");
  // a row of param_tan in the order of the double members of qc_params
  CHECK(PARAM_COUNT == QC_PARAM_COUNT && PT_MU == 0 && PT_MASS == 1 && PT_FZMIN == 2 && PT_FZMAX == 3 && PT_IB == 4, "the scalars and Ib");
  CHECK(PT_S == PT_IB + 9 && PT_W == PT_S + 36 && PT_KFF == PT_W + 144 && PT_KP_P == PT_KFF + 6 && PT_KD_P == PT_KP_P + 3 &&
            PT_KP_W == PT_KD_P + 3 && PT_KD_W == PT_KP_W + 3 && PT_KD_W + 3 == PARAM_COUNT,
        "the matrices and the gains");
  CHECK(sizeof(double) * PARAM_TANGENT_COLD * PARAM_TANGENT_BLOCK == 24576, "the LDS planes of one workgroup");
  for (int e = 0; e < PARAM_COUNT; e++) {  // the layout is the cotangent's: entry e of a row is factor a x factor b of that kernel's record
    const int a = param_factor_a(e), b = param_factor_b(e);
    CHECK(a >= 0 && a < PARAM_RECORD && b >= 0 && b < PARAM_RECORD, "entry %d", e);
    if (e >= PT_S && e < PT_W) CHECK(a == 32 + (e - PT_S) / 6 && b == 38 + (e - PT_S) % 6, "S entry %d is row-major", e);
    if (e >= PT_W && e < PT_KFF) CHECK(a == 44 + (e - PT_W) / 12 && b == 56 + (e - PT_W) % 12, "W entry %d is row-major", e);
  }
}

int main() {
  arguments();
  constants();
  grid_and_layout();
  std::printf("param tangent host logic ok (%ld checks)\n", g_checked);
  return 0;
}
