// The device-free host logic of the legged plant step's reverse pass (quadruped_control_amd/csrc/qc_host.hpp):
// check_leg_plant_adjoint_args through every refusal of qc_leg_plant_step_adjoint_batch, and leg_plant_adjoint_constants - the body's
// constants under this entry point's name, the leg inertia and the call's twenty-five arrays.  Host compiler only - links neither HIP
// nor the library; built with the address and undefined-behaviour sanitizers (__graft_entry__.build_host_test) and run by
// tests/test_leg_plant_adjoint_cpu.py.  Prints the failing case and exits 1 on the first violated check.
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
static int32_t ibuf[4];

typedef qc_leg_plant_adjoint_io Io;
static const double* Io::* const kInputs[] = {&Io::Rwb, &Io::x, &Io::xdot, &Io::w, &Io::joint_q, &Io::joint_qdot, &Io::joint_tau};
static const double* Io::* const kCotangents[] = {&Io::Rwb_next_bar, &Io::x_next_bar,       &Io::xdot_next_bar,
                                                  &Io::w_next_bar,   &Io::joint_q_next_bar, &Io::joint_qdot_next_bar};
static double* Io::* const kOutputs[] = {&Io::Rwb_bar, &Io::x_bar, &Io::xdot_bar, &Io::w_bar, &Io::joint_q_bar, &Io::joint_qdot_bar, &Io::joint_tau_bar};
#define WHO "qc_leg_plant_step_adjoint_batch"

static Io valid_io() {
  Io io{};
  io.struct_size = sizeof(Io);
  for (auto m : kInputs) io.*m = buf;
  io.x_next_bar = buf;
  io.x_bar = buf;
  io.dt = 1.0 / 300.0;
  for (double& v : io.leg_inertia) v = 0.02;
  return io;
}

static void arguments() {
  const qc_handle* const h = reinterpret_cast<const qc_handle*>(buf);  // only compared with null
  const Io io = valid_io();
  CHECK(check_leg_plant_adjoint_args(h, 1, &io) == QC_OK, "the smallest valid call (one cotangent in, one out)");
  {
    Io c = io;
    for (auto m : kCotangents) c.*m = buf;
    for (auto m : kOutputs) c.*m = buf;  // outputs over the cotangents: the aliasing contract, not refused
    c.flags = ibuf;
    CHECK(check_leg_plant_adjoint_args(h, 4097, &c) == QC_OK, "every cotangent and every output");
  }
  const char* const null_arg = WHO ": null argument";
  CHECK_FAILS(check_leg_plant_adjoint_args(nullptr, 1, &io), null_arg, "no handle");
  CHECK_FAILS(check_leg_plant_adjoint_args(h, 1, nullptr), null_arg, "no io");
  CHECK_FAILS(check_leg_plant_adjoint_args(nullptr, 0, &io), null_arg, "no handle, n = 0");
  for (const size_t sz : {(size_t)0, sizeof(Io) - 8, sizeof(Io) + 8, sizeof(qc_leg_plant_io), sizeof(qc_plant_adjoint_io)}) {
    Io c = io;
    c.struct_size = sz;
    char text[320];
    std::snprintf(text, sizeof text,
                  WHO ": qc_leg_plant_adjoint_io.struct_size is %zu, this library's qc_leg_plant_adjoint_io has %zu B (qc_default_leg_plant_adjoint sets it)",
                  sz, sizeof(Io));
    CHECK_FAILS(check_leg_plant_adjoint_args(h, 1, &c), text, "struct_size %zu", sz);
    CHECK_FAILS(check_leg_plant_adjoint_args(h, 0, &c), text, "struct_size %zu, n = 0", sz);
  }
  for (const double dt : {0.0, -0.0, -1.0 / 300.0, kInf, -kInf, kNan}) {
    Io c = io;
    c.dt = dt;
    CHECK_FAILS(check_leg_plant_adjoint_args(h, 1, &c), WHO ": dt must be finite and > 0", "dt %g", dt);
    CHECK_FAILS(check_leg_plant_adjoint_args(h, 0, &c), WHO ": dt must be finite and > 0", "dt %g, n = 0", dt);
  }
  const char* const inertia = WHO ": leg_inertia (hip, thigh, calf) must be finite and > 0; qc_default_leg_plant_adjoint leaves it at 0, the caller gives the step's";
  for (int k = 0; k < 3; k++)
    for (const double v : {0.0, -0.02, kInf, kNan}) {
      Io c = io;
      c.leg_inertia[k] = v;
      CHECK_FAILS(check_leg_plant_adjoint_args(h, 1, &c), inertia, "leg_inertia[%d] %g", k, v);
      CHECK_FAILS(check_leg_plant_adjoint_args(h, 0, &c), inertia, "leg_inertia[%d] %g, n = 0", k, v);
    }
  {
    Io c = io;
    c.x_next_bar = nullptr;
    const char* const none =
        WHO ": no input cotangent given (Rwb_next_bar, x_next_bar, xdot_next_bar, w_next_bar, joint_q_next_bar, joint_qdot_next_bar are all NULL)";
    CHECK_FAILS(check_leg_plant_adjoint_args(h, 1, &c), none, "no cotangent");
    CHECK_FAILS(check_leg_plant_adjoint_args(h, 0, &c), none, "no cotangent, n = 0");
    for (size_t m = 0; m < sizeof(kCotangents) / sizeof(kCotangents[0]); m++) {
      Io one = c;
      one.*kCotangents[m] = buf;
      CHECK(check_leg_plant_adjoint_args(h, 1, &one) == QC_OK, "cotangent %zu alone", m);
    }
  }
  {
    Io c = io;
    c.x_bar = nullptr;
    const char* const none =
        WHO ": no output requested (Rwb_bar, x_bar, xdot_bar, w_bar, joint_q_bar, joint_qdot_bar, joint_tau_bar, flags are all NULL)";
    CHECK_FAILS(check_leg_plant_adjoint_args(h, 1, &c), none, "no output");
    CHECK_FAILS(check_leg_plant_adjoint_args(h, 0, &c), none, "no output, n = 0");
    for (size_t m = 0; m < sizeof(kOutputs) / sizeof(kOutputs[0]); m++) {
      Io one = c;
      one.*kOutputs[m] = buf;
      CHECK(check_leg_plant_adjoint_args(h, 1, &one) == QC_OK, "output %zu alone", m);
    }
    c.flags = ibuf;
    CHECK(check_leg_plant_adjoint_args(h, 1, &c) == QC_OK, "the flags alone");
  }
  const char* const state = WHO ": the state arrays Rwb, x, xdot and w are required";
  const char* const joints = WHO ": joint_q, joint_qdot and joint_tau are required";
  for (size_t m = 0; m < sizeof(kInputs) / sizeof(kInputs[0]); m++) {
    Io c = io;
    c.*kInputs[m] = nullptr;
    CHECK_FAILS(check_leg_plant_adjoint_args(h, 1, &c), m < 4 ? state : joints, "input %zu missing", m);
    CHECK(check_leg_plant_adjoint_args(h, 0, &c) == QC_OK, "input %zu missing, n = 0 asks for no array", m);
  }
  const size_t most = (size_t)0xFFFFFF * LEG_PLANT_BLOCK;
  CHECK(check_leg_plant_adjoint_args(h, most, &io) == QC_OK, "the largest batch of one launch");
  CHECK_FAILS(check_leg_plant_adjoint_args(h, most + 1, &io), WHO ": n is beyond one launch", "one robot more");
  CHECK(sizeof(Io) == 30 * 8, "the io record: struct_size, seven inputs, four contact inputs, six cotangents, eight outputs, leg_inertia and dt");
  CHECK(sizeof(qc_leg_plant_io) == 18 * 8 && sizeof(qc_plant_adjoint_io) == 19 * 8, "the neighbours keep their sizes");
}

static void constants() {
  const double Ib[9] = {0.011253, 0, 0, 0, 0.036203, 0, 0, 0, 0.042673};
  Io io{};
  io.struct_size = sizeof(Io);
  // twenty-five different addresses, so that a swapped pair shows
  const double** in[] = {&io.Rwb, &io.x, &io.xdot, &io.w, &io.joint_q, &io.joint_qdot, &io.joint_tau};
  for (int k = 0; k < 7; k++) *in[k] = buf + k;
  io.stance = reinterpret_cast<const uint8_t*>(buf + 7);
  io.gait_phase = buf + 8;
  io.gait_duty = buf + 9;
  io.cmd_state = reinterpret_cast<const qc_commander_state*>(buf + 10);
  for (int k = 0; k < 6; k++) io.*kCotangents[k] = buf + 11 + k;
  for (int k = 0; k < 7; k++) io.*kOutputs[k] = buf + 17 + k;
  io.flags = ibuf;
  io.dt = 0.002;
  io.leg_inertia[0] = 0.02; io.leg_inertia[1] = 0.03; io.leg_inertia[2] = 0.04;
  LegPlantAdjointArgs a{};
  CHECK(leg_plant_adjoint_constants(9.0, Ib, &io, a) == QC_OK, "the reference's robot");
  PlantArgs p{};
  CHECK(plant_constants(9.0, Ib, 0.002, p) == QC_OK, "the forward step's constants");
  CHECK(a.mass == 9.0 && a.g == PLANT_G && a.dt == 0.002, "mass, g, dt");
  CHECK(a.leg_inertia[0] == 0.02 && a.leg_inertia[1] == 0.03 && a.leg_inertia[2] == 0.04, "the leg inertia");
  for (int k = 0; k < 9; k++) CHECK(a.Ib[k] == p.Ib[k] && a.Ib_inv[k] == p.Ib_inv[k], "Ib and Ib^-1 are the forward step's, entry %d", k);
  CHECK(a.Rwb == buf + 0 && a.x == buf + 1 && a.xdot == buf + 2 && a.w == buf + 3 && a.joint_q == buf + 4 && a.joint_qdot == buf + 5 && a.joint_tau == buf + 6,
        "the inputs");
  CHECK((const void*)a.stance == buf + 7 && a.gait_phase == buf + 8 && a.gait_duty == buf + 9 && (const void*)a.cmd_state == buf + 10, "the contact inputs");
  CHECK(a.Rwb_next_bar == buf + 11 && a.x_next_bar == buf + 12 && a.xdot_next_bar == buf + 13 && a.w_next_bar == buf + 14 &&
            a.joint_q_next_bar == buf + 15 && a.joint_qdot_next_bar == buf + 16,
        "the cotangents");
  CHECK(a.Rwb_bar == buf + 17 && a.x_bar == buf + 18 && a.xdot_bar == buf + 19 && a.w_bar == buf + 20 && a.joint_q_bar == buf + 21 &&
            a.joint_qdot_bar == buf + 22 && a.joint_tau_bar == buf + 23 && a.flags == ibuf,
        "the outputs");
  CHECK(sizeof(LegPlantAdjointArgs) == (21 + 3 + 25) * 8 &&
            reinterpret_cast<const char*>(static_cast<const BodyConst*>(&a)) == reinterpret_cast<const char*>(&a),
        "the body's constants lead the argument struct and the kernarg layout is the flat one");
  for (const double m : {0.0, -1.0, kInf, kNan})
    CHECK_FAILS(leg_plant_adjoint_constants(m, Ib, &io, a), WHO ": the handle's mass is not finite and > 0", "mass %g", m);
  const double zero[9] = {}, asym[9] = {1, 0, 0, 0, 1, 0.25, 0, 0, 1}, nan[9] = {1, 0, 0, 0, kNan, 0, 0, 0, 1}, neg[9] = {1, 0, 0, 0, -1, 0, 0, 0, 1};
  CHECK_FAILS(leg_plant_adjoint_constants(9.0, zero, &io, a), WHO ": the handle's Ib is not positive definite", "zero inertia");
  CHECK_FAILS(leg_plant_adjoint_constants(9.0, neg, &io, a), WHO ": the handle's Ib is not positive definite", "indefinite inertia");
  CHECK_FAILS(leg_plant_adjoint_constants(9.0, asym, &io, a), WHO ": the handle's Ib is not symmetric", "asymmetric inertia");
  CHECK_FAILS(leg_plant_adjoint_constants(9.0, nan, &io, a), WHO ": the handle's Ib is not finite", "NaN inertia");
}

int main() {
  arguments();
  constants();
  std::printf("leg plant adjoint host logic ok (%ld checks)\n", g_checked);
  return 0;
}
