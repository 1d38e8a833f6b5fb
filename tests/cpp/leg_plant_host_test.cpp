// The device-free host logic of the legged plant step (quadruped_control_amd/csrc/qc_host.hpp): the argument check of
// qc_leg_plant_step_batch and the derivation of its kernel's constants, with every message they can give.  Host compiler only -
// links neither HIP nor the library; built with the address and undefined-behaviour sanitizers
// (__graft_entry__.build_leg_plant_host_test) and run by tests/test_leg_plant_cpu.py.  Prints the failing case and exits 1 on the
// first violated check.
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
static qc_leg_plant_io valid_io() {
  qc_leg_plant_io io{};
  io.struct_size = sizeof(qc_leg_plant_io);
  io.Rwb = io.x = io.xdot = io.w = buf;
  io.joint_q = io.joint_qdot = buf;
  io.joint_tau = buf;
  io.leg_inertia[0] = io.leg_inertia[1] = io.leg_inertia[2] = 0.02;
  io.dt = 1.0 / 300.0;
  return io;
}

// ------------------------------------------------------------------------------------------------ (a) check_leg_plant_args
static void arguments() {
  const qc_handle* const h = reinterpret_cast<const qc_handle*>(buf);  // only compared with null
  const qc_leg_plant_io io = valid_io();
  CHECK(check_leg_plant_args(h, 1, &io) == QC_OK, "the smallest valid call (every optional pointer NULL)");
  {
    static uint8_t bytes[4];
    static qc_commander_state cs;
    static int32_t fl;
    qc_leg_plant_io c = io;
    c.stance = bytes; c.gait_phase = buf; c.gait_duty = buf; c.cmd_state = &cs; c.foot_world = buf; c.flags = &fl;
    CHECK(check_leg_plant_args(h, 4097, &c) == QC_OK, "with every optional pointer");
  }
  CHECK_FAILS(check_leg_plant_args(nullptr, 1, &io), "qc_leg_plant_step_batch: null argument", "no handle");
  CHECK_FAILS(check_leg_plant_args(h, 1, nullptr), "qc_leg_plant_step_batch: null argument", "no io");
  for (const size_t sz : {(size_t)0, sizeof(qc_leg_plant_io) - 8, sizeof(qc_leg_plant_io) + 8, sizeof(qc_plant_io)}) {
    qc_leg_plant_io c = io;
    c.struct_size = sz;
    char text[192];
    std::snprintf(text, sizeof(text),
                  "qc_leg_plant_step_batch: qc_leg_plant_io.struct_size is %zu, this library's qc_leg_plant_io has %zu B (qc_default_leg_plant sets it)", sz,
                  sizeof(qc_leg_plant_io));
    CHECK_FAILS(check_leg_plant_args(h, 1, &c), text, "struct_size %zu", sz);
    CHECK_FAILS(check_leg_plant_args(h, 0, &c), text, "struct_size %zu, n = 0", sz);
  }
  const char* const state = "qc_leg_plant_step_batch: the state arrays Rwb, x, xdot and w are required";
  const char* const joints = "qc_leg_plant_step_batch: joint_q, joint_qdot and joint_tau are required";
  {
    double* qc_leg_plant_io::*const st[] = {&qc_leg_plant_io::Rwb, &qc_leg_plant_io::x, &qc_leg_plant_io::xdot, &qc_leg_plant_io::w};
    for (int i = 0; i < 4; i++) {
      qc_leg_plant_io c = io;
      c.*st[i] = nullptr;
      CHECK_FAILS(check_leg_plant_args(h, 1, &c), state, "state array %d missing", i);
      CHECK(check_leg_plant_args(h, 0, &c) == QC_OK, "n = 0 reads no array (state array %d missing)", i);
    }
    double* qc_leg_plant_io::*const jt[] = {&qc_leg_plant_io::joint_q, &qc_leg_plant_io::joint_qdot};
    for (int i = 0; i < 2; i++) {
      qc_leg_plant_io c = io;
      c.*jt[i] = nullptr;
      CHECK_FAILS(check_leg_plant_args(h, 1, &c), joints, "joint array %d missing", i);
    }
    qc_leg_plant_io c = io;
    c.joint_tau = nullptr;
    CHECK_FAILS(check_leg_plant_args(h, 1, &c), joints, "joint_tau missing");
  }
  for (const double dt : {0.0, -0.0, -1.0 / 300.0, kInf, -kInf, kNan}) {
    qc_leg_plant_io c = io;
    c.dt = dt;
    CHECK_FAILS(check_leg_plant_args(h, 1, &c), "qc_leg_plant_step_batch: dt must be finite and > 0", "dt %g", dt);
    CHECK_FAILS(check_leg_plant_args(h, 0, &c), "qc_leg_plant_step_batch: dt must be finite and > 0", "dt %g, n = 0", dt);
  }
  const char* const inertia =
      "qc_leg_plant_step_batch: leg_inertia (hip, thigh, calf) must be finite and > 0; qc_default_leg_plant leaves it at 0, the caller gives it";
  for (const double v : {0.0, -0.0, -0.02, kInf, -kInf, kNan})
    for (int k = 0; k < 3; k++) {
      qc_leg_plant_io c = io;
      c.leg_inertia[k] = v;
      CHECK_FAILS(check_leg_plant_args(h, 1, &c), inertia, "leg_inertia[%d] = %g", k, v);
      CHECK_FAILS(check_leg_plant_args(h, 0, &c), inertia, "leg_inertia[%d] = %g, n = 0", k, v);
    }
  {
    qc_leg_plant_io c = io;
    c.dt = 4.9e-324;
    c.leg_inertia[1] = 4.9e-324;
    CHECK(check_leg_plant_args(h, 1, &c) == QC_OK, "the smallest positive dt and inertia");
  }
  CHECK(check_leg_plant_args(h, (size_t)0xFFFFFF * LEG_PLANT_BLOCK, &io) == QC_OK, "the largest launch");
  CHECK_FAILS(check_leg_plant_args(h, (size_t)0xFFFFFF * LEG_PLANT_BLOCK + 1, &io), "qc_leg_plant_step_batch: n is beyond one launch", "one robot more");
  CHECK(sizeof(qc_leg_plant_io) == 18 * 8, "qc_leg_plant_io is one size field, thirteen pointers, three inertias and dt");
}

// ------------------------------------------------------------------------------------------------ (b) the kernel's constants
static void constants() {
  const double Ib[9] = {0.011253, 0, 0, 0, 0.036203, 0, 0, 0, 0.042673};
  qc_leg_plant_io io = valid_io();
  io.leg_inertia[0] = 0.01; io.leg_inertia[1] = 0.02; io.leg_inertia[2] = 0.03;
  LegPlantArgs a{};
  CHECK(leg_plant_constants(9.0, Ib, &io, a) == QC_OK, "the reference's robot");
  CHECK(a.mass == 9.0 && a.g == 9.81 && a.dt == 1.0 / 300.0, "mass, g, dt travel as given");
  CHECK(a.leg_inertia[0] == 0.01 && a.leg_inertia[1] == 0.02 && a.leg_inertia[2] == 0.03, "leg_inertia travels as given");
  for (int k = 0; k < 9; k++) CHECK(a.Ib[k] == Ib[k], "Ib[%d]", k);
  {
    PlantArgs b{};
    CHECK(plant_constants(9.0, Ib, io.dt, b) == QC_OK, "the plant's own constants");
    for (int k = 0; k < 9; k++) CHECK(a.Ib_inv[k] == b.Ib_inv[k], "the same Ib^-1 as qc_plant_step_batch, entry %d", k);
  }
  // what the existing plant check refuses, under this entry point's name
  for (const double m : {0.0, -1.0, kInf, kNan})
    CHECK_FAILS(leg_plant_constants(m, Ib, &io, a), "qc_leg_plant_step_batch: the handle's mass is not finite and > 0", "mass %g", m);
  {
    const double b[9] = {1, 0, 0, 0, 1, 0.25, 0, 0, 1};
    CHECK_FAILS(leg_plant_constants(9.0, b, &io, a), "qc_leg_plant_step_batch: the handle's Ib is not symmetric", "asymmetric");
  }
  {
    const double b[9] = {1, 2, 0, 2, 1, 0, 0, 0, 1};
    CHECK_FAILS(leg_plant_constants(9.0, b, &io, a), "qc_leg_plant_step_batch: the handle's Ib is not positive definite", "indefinite");
  }
  {
    const double b[9] = {};
    CHECK_FAILS(leg_plant_constants(9.0, b, &io, a), "qc_leg_plant_step_batch: the handle's Ib is not positive definite", "zero (a zeroed qc_params)");
  }
  {
    const double b[9] = {1, 0, 0, 0, kNan, 0, 0, 0, 1};
    CHECK_FAILS(leg_plant_constants(9.0, b, &io, a), "qc_leg_plant_step_batch: the handle's Ib is not finite", "NaN entry");
  }
}

int main() {
  arguments();
  constants();
  std::printf("leg plant host logic ok: %ld checks\n", g_checked);
  return 0;
}
