// The device-free host logic of the plant step's forward mode (quadruped_control_amd/csrc/qc_host.hpp): check_plant_tangent_args
// through every refusal of qc_plant_step_tangent_batch, plant_tangent_constants - the body's constants under this entry point's
// name and the call's seventeen arrays - and plant_tangent_blocks.  Host compiler only - links neither HIP nor the library; built
// with the address and undefined-behaviour sanitizers (__graft_entry__.build_host_test) and run by tests/test_plant_tangent_cpu.py.
// Prints the failing case and exits 1 on the first violated check.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <string>

#include "host_check.hpp"

using namespace qc;

static const double kInf = std::numeric_limits<double>::infinity();
static const double kNan = std::numeric_limits<double>::quiet_NaN();
static double buf[32];

static const double* qc_plant_tangent_io::* const kInputs[] = {&qc_plant_tangent_io::Rwb,      &qc_plant_tangent_io::x,
                                                               &qc_plant_tangent_io::xdot,     &qc_plant_tangent_io::w,
                                                               &qc_plant_tangent_io::grf_body, &qc_plant_tangent_io::foot_world};
static const double* qc_plant_tangent_io::* const kTangents[] = {&qc_plant_tangent_io::Rwb_rot_tan, &qc_plant_tangent_io::x_tan,
                                                                 &qc_plant_tangent_io::xdot_tan,    &qc_plant_tangent_io::w_tan,
                                                                 &qc_plant_tangent_io::grf_tan,     &qc_plant_tangent_io::foot_world_tan};
static double* qc_plant_tangent_io::* const kOutputs[] = {&qc_plant_tangent_io::Rwb_rot_next_tan, &qc_plant_tangent_io::x_next_tan,
                                                          &qc_plant_tangent_io::xdot_next_tan,    &qc_plant_tangent_io::w_next_tan,
                                                          &qc_plant_tangent_io::feet_next_tan};

static qc_plant_tangent_io valid_io() {
  qc_plant_tangent_io io{};
  io.struct_size = sizeof(qc_plant_tangent_io);
  for (auto m : kInputs) io.*m = buf;
  io.x_tan = buf;
  io.x_next_tan = buf;  // over its input: the aliasing contract
  io.dt = 1.0 / 300.0;
  io.n_dir = 1;
  return io;
}

static void arguments() {
  const qc_handle* const h = reinterpret_cast<const qc_handle*>(buf);  // only compared with null
  const qc_plant_tangent_io io = valid_io();
  CHECK(check_plant_tangent_args(h, 1, &io) == QC_OK, "the smallest valid call (one tangent in, one out, in place)");
  {
    qc_plant_tangent_io c = io;
    for (auto m : kTangents) c.*m = buf;
    for (auto m : kOutputs) c.*m = buf;
    c.n_dir = 12;
    CHECK(check_plant_tangent_args(h, 4097, &c) == QC_OK, "every tangent and every output, K = 12");
  }
  const char* const null_arg = "qc_plant_step_tangent_batch: null argument";
  CHECK_FAILS(check_plant_tangent_args(nullptr, 1, &io), null_arg, "no handle");
  CHECK_FAILS(check_plant_tangent_args(h, 1, nullptr), null_arg, "no io");
  CHECK_FAILS(check_plant_tangent_args(nullptr, 0, &io), null_arg, "no handle, n = 0");
  for (const size_t sz : {(size_t)0, sizeof(qc_plant_tangent_io) - 8, sizeof(qc_plant_tangent_io) + 8, sizeof(qc_plant_adjoint_io)}) {
    qc_plant_tangent_io c = io;
    c.struct_size = sz;
    char text[320];
    std::snprintf(text, sizeof text,
                  "qc_plant_step_tangent_batch: qc_plant_tangent_io.struct_size is %zu, this library's qc_plant_tangent_io has %zu B (qc_default_plant_tangent sets it)", sz,
                  sizeof(qc_plant_tangent_io));
    CHECK_FAILS(check_plant_tangent_args(h, 1, &c), text, "struct_size %zu", sz);
    CHECK_FAILS(check_plant_tangent_args(h, 0, &c), text, "struct_size %zu, n = 0", sz);
  }
  for (const double dt : {0.0, -0.0, -1.0 / 300.0, kInf, -kInf, kNan}) {
    qc_plant_tangent_io c = io;
    c.dt = dt;
    CHECK_FAILS(check_plant_tangent_args(h, 1, &c), "qc_plant_step_tangent_batch: dt must be finite and > 0", "dt %g", dt);
    CHECK_FAILS(check_plant_tangent_args(h, 0, &c), "qc_plant_step_tangent_batch: dt must be finite and > 0", "dt %g, n = 0", dt);
  }
  {
    qc_plant_tangent_io c = io;
    c.n_dir = 0;
    CHECK_FAILS(check_plant_tangent_args(h, 1, &c), "qc_plant_step_tangent_batch: n_dir must be >= 1", "n_dir 0");
    CHECK_FAILS(check_plant_tangent_args(h, 0, &c), "qc_plant_step_tangent_batch: n_dir must be >= 1", "n_dir 0, n = 0");
  }
  {
    qc_plant_tangent_io c = io;
    c.x_tan = nullptr;
    const char* const none = "qc_plant_step_tangent_batch: no tangent given (Rwb_rot_tan, x_tan, xdot_tan, w_tan, grf_tan, foot_world_tan are all NULL)";
    CHECK_FAILS(check_plant_tangent_args(h, 1, &c), none, "no tangent");
    CHECK_FAILS(check_plant_tangent_args(h, 0, &c), none, "no tangent, n = 0");
    for (size_t m = 0; m < sizeof(kTangents) / sizeof(kTangents[0]); m++) {
      qc_plant_tangent_io one = c;
      one.*kTangents[m] = buf;
      CHECK(check_plant_tangent_args(h, 1, &one) == QC_OK, "tangent %zu alone", m);
    }
  }
  {
    qc_plant_tangent_io c = io;
    c.x_next_tan = nullptr;
    const char* const none =
        "qc_plant_step_tangent_batch: no output requested (Rwb_rot_next_tan, x_next_tan, xdot_next_tan, w_next_tan, feet_next_tan are all NULL)";
    CHECK_FAILS(check_plant_tangent_args(h, 1, &c), none, "no output");
    CHECK_FAILS(check_plant_tangent_args(h, 0, &c), none, "no output, n = 0");
    for (size_t m = 0; m < sizeof(kOutputs) / sizeof(kOutputs[0]); m++) {
      qc_plant_tangent_io one = c;
      one.*kOutputs[m] = buf;
      CHECK(check_plant_tangent_args(h, 1, &one) == QC_OK, "output %zu alone", m);
    }
  }
  const char* const state = "qc_plant_step_tangent_batch: the state arrays Rwb, x, xdot and w are required";
  const char* const inputs = "qc_plant_step_tangent_batch: grf_body and foot_world are required";
  for (size_t m = 0; m < sizeof(kInputs) / sizeof(kInputs[0]); m++) {
    qc_plant_tangent_io c = io;
    c.*kInputs[m] = nullptr;
    CHECK_FAILS(check_plant_tangent_args(h, 1, &c), m < 4 ? state : inputs, "input %zu missing", m);
    CHECK(check_plant_tangent_args(h, 0, &c) == QC_OK, "input %zu missing, n = 0 asks for no array", m);
  }
  // one lane per (robot, direction): the pairs must fit a launch
  const size_t most = (size_t)0xFFFFFF * PLANT_TANGENT_BLOCK;
  CHECK(check_plant_tangent_args(h, most, &io) == QC_OK, "the largest batch of one launch, K = 1");
  CHECK_FAILS(check_plant_tangent_args(h, most + 1, &io), "qc_plant_step_tangent_batch: n is beyond one launch", "one robot more");
  {
    qc_plant_tangent_io c = io;
    c.n_dir = 64;
    CHECK(check_plant_tangent_args(h, (size_t)0xFFFFFF, &c) == QC_OK, "the largest n * n_dir, K = 64");
    CHECK_FAILS(check_plant_tangent_args(h, (size_t)0xFFFFFF + 1, &c), "qc_plant_step_tangent_batch: n * n_dir is beyond one launch", "one robot more at K = 64");
    c.n_dir = most;
    CHECK(check_plant_tangent_args(h, 1, &c) == QC_OK, "one robot, the most directions");
    c.n_dir = most + 1;
    CHECK_FAILS(check_plant_tangent_args(h, 1, &c), "qc_plant_step_tangent_batch: n * n_dir is beyond one launch", "one direction more");
    c.n_dir = std::numeric_limits<size_t>::max();  // (a product that would wrap)
    CHECK_FAILS(check_plant_tangent_args(h, 3, &c), "qc_plant_step_tangent_batch: n * n_dir is beyond one launch", "n_dir = SIZE_MAX");
    CHECK(check_plant_tangent_args(h, 0, &c) == QC_OK, "n = 0 launches nothing whatever n_dir is");
  }
  CHECK(sizeof(qc_plant_tangent_io) == 20 * 8, "the io record: struct_size, six inputs, dt, n_dir, six tangents, five outputs");
  CHECK(sizeof(qc_tangent_io) == 17 * 8 && sizeof(qc_plant_io) == 9 * 8 && sizeof(qc_plant_adjoint_io) == 19 * 8, "the other records keep their sizes");
}

static void constants() {
  const double Ib[9] = {0.011253, 0, 0, 0, 0.036203, 0, 0, 0, 0.042673};
  qc_plant_tangent_io io{};
  io.struct_size = sizeof(qc_plant_tangent_io);
  // seventeen different addresses, so that a swapped pair shows
  io.Rwb = buf + 0; io.x = buf + 1; io.xdot = buf + 2; io.w = buf + 3; io.grf_body = buf + 4; io.foot_world = buf + 5;
  io.Rwb_rot_tan = buf + 6; io.x_tan = buf + 7; io.xdot_tan = buf + 8; io.w_tan = buf + 9; io.grf_tan = buf + 10; io.foot_world_tan = buf + 11;
  io.Rwb_rot_next_tan = buf + 12; io.x_next_tan = buf + 13; io.xdot_next_tan = buf + 14; io.w_next_tan = buf + 15; io.feet_next_tan = buf + 16;
  io.dt = 0.002;
  io.n_dir = 7;
  PlantTangentArgs a{};
  CHECK(plant_tangent_constants(9.0, Ib, &io, a) == QC_OK, "the reference's robot");
  PlantArgs p{};
  CHECK(plant_constants(9.0, Ib, 0.002, p) == QC_OK, "the forward step's constants");
  CHECK(a.mass == 9.0 && a.g == PLANT_G && a.dt == 0.002 && a.n_dir == 7, "mass, g, dt, K");
  for (int k = 0; k < 9; k++) CHECK(a.Ib[k] == p.Ib[k] && a.Ib_inv[k] == p.Ib_inv[k], "Ib and Ib^-1 are the forward step's, entry %d", k);
  CHECK(a.Rwb == buf + 0 && a.x == buf + 1 && a.xdot == buf + 2 && a.w == buf + 3 && a.grf_body == buf + 4 && a.foot_world == buf + 5, "the inputs");
  CHECK(a.Rwb_rot_tan == buf + 6 && a.x_tan == buf + 7 && a.xdot_tan == buf + 8 && a.w_tan == buf + 9 && a.grf_tan == buf + 10 && a.foot_world_tan == buf + 11,
        "the tangents");
  CHECK(a.Rwb_rot_next_tan == buf + 12 && a.x_next_tan == buf + 13 && a.xdot_next_tan == buf + 14 && a.w_next_tan == buf + 15 && a.feet_next_tan == buf + 16,
        "the outputs");
  CHECK(sizeof(PlantTangentArgs) == (21 + 18) * 8 &&
            reinterpret_cast<const char*>(static_cast<const BodyConst*>(&a)) == reinterpret_cast<const char*>(&a),
        "the body's constants lead the argument struct and the kernarg layout is the flat one");
  for (const double m : {0.0, -1.0, kInf, kNan})
    CHECK_FAILS(plant_tangent_constants(m, Ib, &io, a), "qc_plant_step_tangent_batch: the handle's mass is not finite and > 0", "mass %g", m);
  const double zero[9] = {}, asym[9] = {1, 0, 0, 0, 1, 0.25, 0, 0, 1}, nan[9] = {1, 0, 0, 0, kNan, 0, 0, 0, 1}, neg[9] = {1, 0, 0, 0, -1, 0, 0, 0, 1};
  CHECK_FAILS(plant_tangent_constants(9.0, zero, &io, a), "qc_plant_step_tangent_batch: the handle's Ib is not positive definite", "zero inertia");
  CHECK_FAILS(plant_tangent_constants(9.0, neg, &io, a), "qc_plant_step_tangent_batch: the handle's Ib is not positive definite", "indefinite inertia");
  CHECK_FAILS(plant_tangent_constants(9.0, asym, &io, a), "qc_plant_step_tangent_batch: the handle's Ib is not symmetric", "asymmetric inertia");
  CHECK_FAILS(plant_tangent_constants(9.0, nan, &io, a), "qc_plant_step_tangent_batch: the handle's Ib is not finite", "NaN inertia");
}

static void blocks() {
  CHECK(plant_tangent_blocks(1, 1) == 1 && plant_tangent_blocks(64, 1) == 1 && plant_tangent_blocks(65, 1) == 2, "one wave of pairs per workgroup");
  CHECK(plant_tangent_blocks(22, 3) == 2 && plant_tangent_blocks(64, 12) == 12, "K multiplies the pairs");
  const size_t cap = (size_t)PLANT_TANGENT_MAX_BLOCKS * PLANT_TANGENT_BLOCK;
  CHECK(plant_tangent_blocks(cap, 1) == PLANT_TANGENT_MAX_BLOCKS && plant_tangent_blocks(cap + 1, 1) == PLANT_TANGENT_MAX_BLOCKS &&
            plant_tangent_blocks(cap / 4 + 1, 4) == PLANT_TANGENT_MAX_BLOCKS && plant_tangent_blocks(cap - 64, 1) == PLANT_TANGENT_MAX_BLOCKS - 1,
        "the grid cap: the waves stride beyond it");
}

int main() {
  arguments();
  constants();
  blocks();
  std::printf("plant tangent host logic ok (%ld checks)\n", g_checked);
  return 0;
}
