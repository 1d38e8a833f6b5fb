// The device-free host logic of the legged plant step's forward mode (quadruped_control_amd/csrc/qc_host.hpp):
// check_leg_plant_tangent_args through every refusal of qc_leg_plant_step_tangent_batch, leg_plant_tangent_constants - the body's
// constants under this entry point's name, the leg inertia and the call's arrays - and leg_plant_tangent_blocks.  Host compiler only
// - links neither HIP nor the library; built with the address and undefined-behaviour sanitizers (__graft_entry__.build_host_test)
// and run by tests/test_leg_plant_tangent_cpu.py.  Prints the failing case and exits 1 on the first violated check.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <string>

#include "host_check.hpp"

using namespace qc;

static const double kInf = std::numeric_limits<double>::infinity();
static const double kNan = std::numeric_limits<double>::quiet_NaN();
static double buf[40];
static int32_t ibuf[4];
static uint8_t bbuf[4];

using Io = qc_leg_plant_tangent_io;
static const double* Io::* const kInputs[] = {&Io::Rwb, &Io::x, &Io::xdot, &Io::w, &Io::joint_q, &Io::joint_qdot, &Io::joint_tau};
static const double* Io::* const kTangents[] = {&Io::Rwb_rot_tan, &Io::x_tan, &Io::xdot_tan, &Io::w_tan, &Io::joint_q_tan, &Io::joint_qdot_tan, &Io::joint_tau_tan};
static double* Io::* const kOutputs[] = {&Io::Rwb_rot_next_tan, &Io::x_next_tan, &Io::xdot_next_tan, &Io::w_next_tan, &Io::joint_q_next_tan, &Io::joint_qdot_next_tan};

static Io valid_io() {
  Io io{};
  io.struct_size = sizeof(Io);
  for (auto m : kInputs) io.*m = buf;
  io.x_tan = buf;
  io.x_next_tan = buf;  // over its input: the aliasing contract
  io.dt = 1.0 / 300.0;
  io.n_dir = 1;
  for (int k = 0; k < 3; k++) io.leg_inertia[k] = 0.02 + 0.005 * k;
  return io;
}

static void arguments() {
  const qc_handle* const h = reinterpret_cast<const qc_handle*>(buf);  // only compared with null
  const Io io = valid_io();
  const char* const who = "qc_leg_plant_step_tangent_batch";
  const auto msg = [who](const char* what) { return std::string(who) + what; };
  CHECK(check_leg_plant_tangent_args(h, 1, &io) == QC_OK, "the smallest valid call (one tangent in, one out, in place)");
  {
    Io c = io;
    for (auto m : kTangents) c.*m = buf;
    for (auto m : kOutputs) c.*m = buf;
    c.flags = ibuf;
    c.stance = bbuf;
    c.n_dir = 36;
    CHECK(check_leg_plant_tangent_args(h, 4097, &c) == QC_OK, "every tangent and every output, K = 36");
  }
  CHECK_FAILS(check_leg_plant_tangent_args(nullptr, 1, &io), msg(": null argument"), "no handle");
  CHECK_FAILS(check_leg_plant_tangent_args(h, 1, nullptr), msg(": null argument"), "no io");
  CHECK_FAILS(check_leg_plant_tangent_args(nullptr, 0, &io), msg(": null argument"), "no handle, n = 0");
  for (const size_t sz : {(size_t)0, sizeof(Io) - 8, sizeof(Io) + 8, sizeof(qc_leg_plant_adjoint_io)}) {
    Io c = io;
    c.struct_size = sz;
    char text[320];
    std::snprintf(text, sizeof text,
                  "%s: qc_leg_plant_tangent_io.struct_size is %zu, this library's qc_leg_plant_tangent_io has %zu B (qc_default_leg_plant_tangent sets it)", who, sz,
                  sizeof(Io));
    CHECK_FAILS(check_leg_plant_tangent_args(h, 1, &c), text, "struct_size %zu", sz);
    CHECK_FAILS(check_leg_plant_tangent_args(h, 0, &c), text, "struct_size %zu, n = 0", sz);
  }
  for (const double dt : {0.0, -0.0, -1.0 / 300.0, kInf, -kInf, kNan}) {
    Io c = io;
    c.dt = dt;
    CHECK_FAILS(check_leg_plant_tangent_args(h, 1, &c), msg(": dt must be finite and > 0"), "dt %g", dt);
    CHECK_FAILS(check_leg_plant_tangent_args(h, 0, &c), msg(": dt must be finite and > 0"), "dt %g, n = 0", dt);
  }
  const auto inertia = msg(": leg_inertia (hip, thigh, calf) must be finite and > 0; qc_default_leg_plant_tangent leaves it at 0, the caller gives the step's");
  for (int k = 0; k < 3; k++)
    for (const double v : {0.0, -0.02, kInf, kNan}) {
      Io c = io;
      c.leg_inertia[k] = v;
      CHECK_FAILS(check_leg_plant_tangent_args(h, 1, &c), inertia, "leg_inertia[%d] = %g", k, v);
      CHECK_FAILS(check_leg_plant_tangent_args(h, 0, &c), inertia, "leg_inertia[%d] = %g, n = 0", k, v);
    }
  {
    Io c = io;
    for (int k = 0; k < 3; k++) c.leg_inertia[k] = 0.0;  // as the default leaves it
    CHECK_FAILS(check_leg_plant_tangent_args(h, 1, &c), inertia, "the default's leg_inertia");
  }
  {
    Io c = io;
    c.n_dir = 0;
    CHECK_FAILS(check_leg_plant_tangent_args(h, 1, &c), msg(": n_dir must be >= 1"), "n_dir 0");
    CHECK_FAILS(check_leg_plant_tangent_args(h, 0, &c), msg(": n_dir must be >= 1"), "n_dir 0, n = 0");
  }
  {
    Io c = io;
    c.x_tan = nullptr;
    const auto none = msg(": no tangent given (Rwb_rot_tan, x_tan, xdot_tan, w_tan, joint_q_tan, joint_qdot_tan, joint_tau_tan are all NULL)");
    CHECK_FAILS(check_leg_plant_tangent_args(h, 1, &c), none, "no tangent");
    CHECK_FAILS(check_leg_plant_tangent_args(h, 0, &c), none, "no tangent, n = 0");
    for (size_t m = 0; m < sizeof(kTangents) / sizeof(kTangents[0]); m++) {
      Io one = c;
      one.*kTangents[m] = buf;
      CHECK(check_leg_plant_tangent_args(h, 1, &one) == QC_OK, "tangent %zu alone", m);
    }
  }
  {
    Io c = io;
    c.x_next_tan = nullptr;
    const auto none =
        msg(": no output requested (Rwb_rot_next_tan, x_next_tan, xdot_next_tan, w_next_tan, joint_q_next_tan, joint_qdot_next_tan, flags are all NULL)");
    CHECK_FAILS(check_leg_plant_tangent_args(h, 1, &c), none, "no output");
    CHECK_FAILS(check_leg_plant_tangent_args(h, 0, &c), none, "no output, n = 0");
    for (size_t m = 0; m < sizeof(kOutputs) / sizeof(kOutputs[0]); m++) {
      Io one = c;
      one.*kOutputs[m] = buf;
      CHECK(check_leg_plant_tangent_args(h, 1, &one) == QC_OK, "output %zu alone", m);
    }
    c.flags = ibuf;
    CHECK(check_leg_plant_tangent_args(h, 1, &c) == QC_OK, "flags alone");
  }
  for (size_t m = 0; m < sizeof(kInputs) / sizeof(kInputs[0]); m++) {
    Io c = io;
    c.*kInputs[m] = nullptr;
    CHECK_FAILS(check_leg_plant_tangent_args(h, 1, &c),
                m < 4 ? msg(": the state arrays Rwb, x, xdot and w are required") : msg(": joint_q, joint_qdot and joint_tau are required"), "input %zu missing", m);
    CHECK(check_leg_plant_tangent_args(h, 0, &c) == QC_OK, "input %zu missing, n = 0 asks for no array", m);
  }
  // one lane per (robot, direction): the pairs must fit a launch
  const size_t most = (size_t)0xFFFFFF * LEG_PLANT_TANGENT_BLOCK;
  CHECK(check_leg_plant_tangent_args(h, most, &io) == QC_OK, "the largest batch of one launch, K = 1");
  CHECK_FAILS(check_leg_plant_tangent_args(h, most + 1, &io), msg(": n is beyond one launch"), "one robot more");
  {
    Io c = io;
    c.n_dir = 64;
    CHECK(check_leg_plant_tangent_args(h, (size_t)0xFFFFFF, &c) == QC_OK, "the largest n * n_dir, K = 64");
    CHECK_FAILS(check_leg_plant_tangent_args(h, (size_t)0xFFFFFF + 1, &c), msg(": n * n_dir is beyond one launch"), "one robot more at K = 64");
    c.n_dir = most + 1;
    CHECK_FAILS(check_leg_plant_tangent_args(h, 1, &c), msg(": n * n_dir is beyond one launch"), "one direction more");
    c.n_dir = std::numeric_limits<size_t>::max();  // (a product that would wrap)
    CHECK_FAILS(check_leg_plant_tangent_args(h, 3, &c), msg(": n * n_dir is beyond one launch"), "n_dir = SIZE_MAX");
    CHECK(check_leg_plant_tangent_args(h, 0, &c) == QC_OK, "n = 0 launches nothing whatever n_dir is");
  }
  CHECK(sizeof(Io) == 31 * 8, "the io record: struct_size, seven inputs, four contact inputs, leg_inertia[3], dt, n_dir, seven tangents, six outputs, flags");
  CHECK(sizeof(qc_tangent_io) == 17 * 8 && sizeof(qc_plant_tangent_io) == 20 * 8 && sizeof(qc_torque_tangent_io) == 7 * 8, "the other records keep their sizes");
}

static void constants() {
  const double Ib[9] = {0.011253, 0, 0, 0, 0.036203, 0, 0, 0, 0.042673};
  Io io{};
  io.struct_size = sizeof(Io);
  // different addresses, so that a swapped pair shows
  io.Rwb = buf + 0; io.x = buf + 1; io.xdot = buf + 2; io.w = buf + 3; io.joint_q = buf + 4; io.joint_qdot = buf + 5; io.joint_tau = buf + 6;
  io.stance = bbuf; io.gait_phase = buf + 7; io.gait_duty = buf + 8; io.cmd_state = reinterpret_cast<const qc_commander_state*>(buf + 9);
  io.Rwb_rot_tan = buf + 10; io.x_tan = buf + 11; io.xdot_tan = buf + 12; io.w_tan = buf + 13; io.joint_q_tan = buf + 14; io.joint_qdot_tan = buf + 15;
  io.joint_tau_tan = buf + 16;
  io.Rwb_rot_next_tan = buf + 17; io.x_next_tan = buf + 18; io.xdot_next_tan = buf + 19; io.w_next_tan = buf + 20; io.joint_q_next_tan = buf + 21;
  io.joint_qdot_next_tan = buf + 22; io.flags = ibuf;
  io.leg_inertia[0] = 0.02; io.leg_inertia[1] = 0.03; io.leg_inertia[2] = 0.025;
  io.dt = 0.002;
  io.n_dir = 36;
  LegPlantTangentArgs a{};
  CHECK(leg_plant_tangent_constants(9.0, Ib, &io, a) == QC_OK, "the reference's robot");
  PlantArgs p{};
  CHECK(plant_constants(9.0, Ib, 0.002, p) == QC_OK, "the forward step's constants");
  CHECK(a.mass == 9.0 && a.g == PLANT_G && a.dt == 0.002 && a.n_dir == 36, "mass, g, dt, K");
  CHECK(a.leg_inertia[0] == 0.02 && a.leg_inertia[1] == 0.03 && a.leg_inertia[2] == 0.025, "the leg inertia");
  for (int k = 0; k < 9; k++) CHECK(a.Ib[k] == p.Ib[k] && a.Ib_inv[k] == p.Ib_inv[k], "Ib and Ib^-1 are the forward step's, entry %d", k);
  CHECK(a.Rwb == buf + 0 && a.x == buf + 1 && a.xdot == buf + 2 && a.w == buf + 3 && a.joint_q == buf + 4 && a.joint_qdot == buf + 5 && a.joint_tau == buf + 6, "the inputs");
  CHECK(a.stance == bbuf && a.gait_phase == buf + 7 && a.gait_duty == buf + 8 && reinterpret_cast<const double*>(a.cmd_state) == buf + 9, "the contact inputs");
  CHECK(a.Rwb_rot_tan == buf + 10 && a.x_tan == buf + 11 && a.xdot_tan == buf + 12 && a.w_tan == buf + 13 && a.joint_q_tan == buf + 14 && a.joint_qdot_tan == buf + 15 &&
            a.joint_tau_tan == buf + 16,
        "the tangents");
  CHECK(a.Rwb_rot_next_tan == buf + 17 && a.x_next_tan == buf + 18 && a.xdot_next_tan == buf + 19 && a.w_next_tan == buf + 20 && a.joint_q_next_tan == buf + 21 &&
            a.joint_qdot_next_tan == buf + 22 && a.flags == ibuf,
        "the outputs");
  CHECK(sizeof(LegPlantTangentArgs) == (21 + 3 + 7 + 4 + 1 + 7 + 6 + 1) * 8 &&
            reinterpret_cast<const char*>(static_cast<const BodyConst*>(&a)) == reinterpret_cast<const char*>(&a),
        "the body's constants lead the argument struct and the kernarg layout is the flat one");
  for (const double m : {0.0, -1.0, kInf, kNan})
    CHECK_FAILS(leg_plant_tangent_constants(m, Ib, &io, a), "qc_leg_plant_step_tangent_batch: the handle's mass is not finite and > 0", "mass %g", m);
  const double zero[9] = {}, asym[9] = {1, 0, 0, 0, 1, 0.25, 0, 0, 1}, nan[9] = {1, 0, 0, 0, kNan, 0, 0, 0, 1}, neg[9] = {1, 0, 0, 0, -1, 0, 0, 0, 1};
  CHECK_FAILS(leg_plant_tangent_constants(9.0, zero, &io, a), "qc_leg_plant_step_tangent_batch: the handle's Ib is not positive definite", "zero inertia");
  CHECK_FAILS(leg_plant_tangent_constants(9.0, neg, &io, a), "qc_leg_plant_step_tangent_batch: the handle's Ib is not positive definite", "indefinite inertia");
  CHECK_FAILS(leg_plant_tangent_constants(9.0, asym, &io, a), "qc_leg_plant_step_tangent_batch: the handle's Ib is not symmetric", "asymmetric inertia");
  CHECK_FAILS(leg_plant_tangent_constants(9.0, nan, &io, a), "qc_leg_plant_step_tangent_batch: the handle's Ib is not finite", "NaN inertia");
}

static void blocks() {
  CHECK(leg_plant_tangent_blocks(1, 1) == 1 && leg_plant_tangent_blocks(64, 1) == 1 && leg_plant_tangent_blocks(65, 1) == 2, "one wave of pairs per workgroup");
  CHECK(leg_plant_tangent_blocks(22, 3) == 2 && leg_plant_tangent_blocks(64, 36) == 36, "K multiplies the pairs");
  const size_t cap = (size_t)LEG_PLANT_TANGENT_MAX_BLOCKS * LEG_PLANT_TANGENT_BLOCK;
  CHECK(leg_plant_tangent_blocks(cap, 1) == LEG_PLANT_TANGENT_MAX_BLOCKS && leg_plant_tangent_blocks(cap + 1, 1) == LEG_PLANT_TANGENT_MAX_BLOCKS &&
            leg_plant_tangent_blocks(cap / 4 + 1, 4) == LEG_PLANT_TANGENT_MAX_BLOCKS && leg_plant_tangent_blocks(cap - 64, 1) == LEG_PLANT_TANGENT_MAX_BLOCKS - 1,
        "the grid cap: the waves stride beyond it");
}

int main() {
  arguments();
  constants();
  blocks();
  std::printf("leg plant tangent host logic ok (%ld checks)\n", g_checked);
  return 0;
}
