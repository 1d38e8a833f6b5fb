// The device-free host logic of the plant step's reverse pass (quadruped_control_amd/csrc/qc_host.hpp): check_plant_adjoint_args
// through every refusal of qc_plant_step_adjoint_batch, and plant_adjoint_constants - the body's constants under this entry point's
// name and the call's seventeen arrays.  Host compiler only - links neither HIP nor the library; built with the address and
// undefined-behaviour sanitizers (__graft_entry__.build_host_test) and run by tests/test_plant_adjoint_cpu.py.  Prints the failing
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
static double buf[32];

static const double* qc_plant_adjoint_io::* const kInputs[] = {&qc_plant_adjoint_io::Rwb,      &qc_plant_adjoint_io::x,
                                                               &qc_plant_adjoint_io::xdot,     &qc_plant_adjoint_io::w,
                                                               &qc_plant_adjoint_io::grf_body, &qc_plant_adjoint_io::foot_world};
static const double* qc_plant_adjoint_io::* const kCotangents[] = {&qc_plant_adjoint_io::Rwb_next_bar, &qc_plant_adjoint_io::x_next_bar,
                                                                   &qc_plant_adjoint_io::xdot_next_bar, &qc_plant_adjoint_io::w_next_bar,
                                                                   &qc_plant_adjoint_io::feet_next_bar};
static double* qc_plant_adjoint_io::* const kOutputs[] = {&qc_plant_adjoint_io::Rwb_bar, &qc_plant_adjoint_io::x_bar,   &qc_plant_adjoint_io::xdot_bar,
                                                          &qc_plant_adjoint_io::w_bar,   &qc_plant_adjoint_io::grf_bar, &qc_plant_adjoint_io::foot_world_bar};

static qc_plant_adjoint_io valid_io() {
  qc_plant_adjoint_io io{};
  io.struct_size = sizeof(qc_plant_adjoint_io);
  for (auto m : kInputs) io.*m = buf;
  io.x_next_bar = buf;
  io.x_bar = buf;
  io.dt = 1.0 / 300.0;
  return io;
}

static void arguments() {
  const qc_handle* const h = reinterpret_cast<const qc_handle*>(buf);  // only compared with null
  const qc_plant_adjoint_io io = valid_io();
  CHECK(check_plant_adjoint_args(h, 1, &io) == QC_OK, "the smallest valid call (one cotangent in, one out)");
  {
    qc_plant_adjoint_io c = io;
    for (auto m : kCotangents) c.*m = buf;
    for (auto m : kOutputs) c.*m = buf;  // outputs over the cotangents: the aliasing contract, not refused
    CHECK(check_plant_adjoint_args(h, 4097, &c) == QC_OK, "every cotangent and every output");
  }
  const char* const null_arg = "qc_plant_step_adjoint_batch: null argument";
  CHECK_FAILS(check_plant_adjoint_args(nullptr, 1, &io), null_arg, "no handle");
  CHECK_FAILS(check_plant_adjoint_args(h, 1, nullptr), null_arg, "no io");
  CHECK_FAILS(check_plant_adjoint_args(nullptr, 0, &io), null_arg, "no handle, n = 0");
  for (const size_t sz : {(size_t)0, sizeof(qc_plant_adjoint_io) - 8, sizeof(qc_plant_adjoint_io) + 8, sizeof(qc_plant_io)}) {
    qc_plant_adjoint_io c = io;
    c.struct_size = sz;
    char text[320];
    std::snprintf(text, sizeof text,
                  "qc_plant_step_adjoint_batch: qc_plant_adjoint_io.struct_size is %zu, this library's qc_plant_adjoint_io has %zu B (qc_default_plant_adjoint sets it)", sz,
                  sizeof(qc_plant_adjoint_io));
    CHECK_FAILS(check_plant_adjoint_args(h, 1, &c), text, "struct_size %zu", sz);
    CHECK_FAILS(check_plant_adjoint_args(h, 0, &c), text, "struct_size %zu, n = 0", sz);
  }
  for (const double dt : {0.0, -0.0, -1.0 / 300.0, kInf, -kInf, kNan}) {
    qc_plant_adjoint_io c = io;
    c.dt = dt;
    CHECK_FAILS(check_plant_adjoint_args(h, 1, &c), "qc_plant_step_adjoint_batch: dt must be finite and > 0", "dt %g", dt);
    CHECK_FAILS(check_plant_adjoint_args(h, 0, &c), "qc_plant_step_adjoint_batch: dt must be finite and > 0", "dt %g, n = 0", dt);
  }
  {
    qc_plant_adjoint_io c = io;
    c.x_next_bar = nullptr;
    const char* const none =
        "qc_plant_step_adjoint_batch: no input cotangent given (Rwb_next_bar, x_next_bar, xdot_next_bar, w_next_bar, feet_next_bar are all NULL)";
    CHECK_FAILS(check_plant_adjoint_args(h, 1, &c), none, "no cotangent");
    CHECK_FAILS(check_plant_adjoint_args(h, 0, &c), none, "no cotangent, n = 0");
    for (size_t m = 0; m < sizeof(kCotangents) / sizeof(kCotangents[0]); m++) {
      qc_plant_adjoint_io one = c;
      one.*kCotangents[m] = buf;
      CHECK(check_plant_adjoint_args(h, 1, &one) == QC_OK, "cotangent %zu alone", m);
    }
  }
  {
    qc_plant_adjoint_io c = io;
    c.x_bar = nullptr;
    const char* const none = "qc_plant_step_adjoint_batch: no output requested (Rwb_bar, x_bar, xdot_bar, w_bar, grf_bar, foot_world_bar are all NULL)";
    CHECK_FAILS(check_plant_adjoint_args(h, 1, &c), none, "no output");
    CHECK_FAILS(check_plant_adjoint_args(h, 0, &c), none, "no output, n = 0");
    for (size_t m = 0; m < sizeof(kOutputs) / sizeof(kOutputs[0]); m++) {
      qc_plant_adjoint_io one = c;
      one.*kOutputs[m] = buf;
      CHECK(check_plant_adjoint_args(h, 1, &one) == QC_OK, "output %zu alone", m);
    }
  }
  const char* const state = "qc_plant_step_adjoint_batch: the state arrays Rwb, x, xdot and w are required";
  const char* const inputs = "qc_plant_step_adjoint_batch: grf_body and foot_world are required";
  for (size_t m = 0; m < sizeof(kInputs) / sizeof(kInputs[0]); m++) {
    qc_plant_adjoint_io c = io;
    c.*kInputs[m] = nullptr;
    CHECK_FAILS(check_plant_adjoint_args(h, 1, &c), m < 4 ? state : inputs, "input %zu missing", m);
    CHECK(check_plant_adjoint_args(h, 0, &c) == QC_OK, "input %zu missing, n = 0 asks for no array", m);
  }
  const size_t most = (size_t)0xFFFFFF * PLANT_BLOCK;
  CHECK(check_plant_adjoint_args(h, most, &io) == QC_OK, "the largest batch of one launch");
  CHECK_FAILS(check_plant_adjoint_args(h, most + 1, &io), "qc_plant_step_adjoint_batch: n is beyond one launch", "one robot more");
  CHECK(sizeof(qc_plant_adjoint_io) == 19 * 8, "the io record: struct_size, six inputs, five cotangents, six outputs and dt");
  CHECK(sizeof(qc_plant_io) == 9 * 8, "qc_plant_io keeps its size");
}

static void constants() {
  const double Ib[9] = {0.011253, 0, 0, 0, 0.036203, 0, 0, 0, 0.042673};
  qc_plant_adjoint_io io{};
  io.struct_size = sizeof(qc_plant_adjoint_io);
  // seventeen different addresses, so that a swapped pair shows
  io.Rwb = buf + 0; io.x = buf + 1; io.xdot = buf + 2; io.w = buf + 3; io.grf_body = buf + 4; io.foot_world = buf + 5;
  io.Rwb_next_bar = buf + 6; io.x_next_bar = buf + 7; io.xdot_next_bar = buf + 8; io.w_next_bar = buf + 9; io.feet_next_bar = buf + 10;
  io.Rwb_bar = buf + 11; io.x_bar = buf + 12; io.xdot_bar = buf + 13; io.w_bar = buf + 14; io.grf_bar = buf + 15; io.foot_world_bar = buf + 16;
  io.dt = 0.002;
  PlantAdjointArgs a{};
  CHECK(plant_adjoint_constants(9.0, Ib, &io, a) == QC_OK, "the reference's robot");
  PlantArgs p{};
  CHECK(plant_constants(9.0, Ib, 0.002, p) == QC_OK, "the forward step's constants");
  CHECK(a.mass == 9.0 && a.g == PLANT_G && a.dt == 0.002, "mass, g, dt");
  for (int k = 0; k < 9; k++) CHECK(a.Ib[k] == p.Ib[k] && a.Ib_inv[k] == p.Ib_inv[k], "Ib and Ib^-1 are the forward step's, entry %d", k);
  CHECK(a.Rwb == buf + 0 && a.x == buf + 1 && a.xdot == buf + 2 && a.w == buf + 3 && a.grf_body == buf + 4 && a.foot_world == buf + 5, "the inputs");
  CHECK(a.Rwb_next_bar == buf + 6 && a.x_next_bar == buf + 7 && a.xdot_next_bar == buf + 8 && a.w_next_bar == buf + 9 && a.feet_next_bar == buf + 10,
        "the cotangents");
  CHECK(a.Rwb_bar == buf + 11 && a.x_bar == buf + 12 && a.xdot_bar == buf + 13 && a.w_bar == buf + 14 && a.grf_bar == buf + 15 &&
            a.foot_world_bar == buf + 16,
        "the outputs");
  CHECK(sizeof(PlantAdjointArgs) == (21 + 17) * 8 &&
            reinterpret_cast<const char*>(static_cast<const BodyConst*>(&a)) == reinterpret_cast<const char*>(&a),
        "the body's constants lead the argument struct and the kernarg layout is the flat one");
  for (const double m : {0.0, -1.0, kInf, kNan})
    CHECK_FAILS(plant_adjoint_constants(m, Ib, &io, a), "qc_plant_step_adjoint_batch: the handle's mass is not finite and > 0", "mass %g", m);
  const double zero[9] = {}, asym[9] = {1, 0, 0, 0, 1, 0.25, 0, 0, 1}, nan[9] = {1, 0, 0, 0, kNan, 0, 0, 0, 1}, neg[9] = {1, 0, 0, 0, -1, 0, 0, 0, 1};
  CHECK_FAILS(plant_adjoint_constants(9.0, zero, &io, a), "qc_plant_step_adjoint_batch: the handle's Ib is not positive definite", "zero inertia");
  CHECK_FAILS(plant_adjoint_constants(9.0, neg, &io, a), "qc_plant_step_adjoint_batch: the handle's Ib is not positive definite", "indefinite inertia");
  CHECK_FAILS(plant_adjoint_constants(9.0, asym, &io, a), "qc_plant_step_adjoint_batch: the handle's Ib is not symmetric", "asymmetric inertia");
  CHECK_FAILS(plant_adjoint_constants(9.0, nan, &io, a), "qc_plant_step_adjoint_batch: the handle's Ib is not finite", "NaN inertia");
}

int main() {
  arguments();
  constants();
  std::printf("plant adjoint host logic ok (%ld checks)\n", g_checked);
  return 0;
}
