// The device-free host logic of the torque map's forward mode (quadruped_control_amd/csrc/qc_host.hpp): check_torque_tangent_args
// through every refusal of qc_torque_tangent_batch, torque_tangent_constants - the ten kernel arguments - and torque_tangent_blocks.
// Host compiler only - links neither HIP nor the library; built with the address and undefined-behaviour sanitizers
// (__graft_entry__.build_host_test) and run by tests/test_leg_plant_tangent_cpu.py.  Prints the failing case and exits 1 on the
// first violated check.
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <string>

#include "host_check.hpp"

using namespace qc;

static double buf[32];
static int32_t ibuf[4];
static uint8_t bbuf[4];

static qc_torque_tangent_io valid_io() {
  qc_torque_tangent_io io{};
  io.struct_size = sizeof(qc_torque_tangent_io);
  io.grf_body = buf;
  io.status = ibuf;
  io.n_dir = 1;
  io.grf_tan = buf;
  io.joint_tau_tan = buf;  // over its input: the aliasing contract
  return io;
}

static void arguments() {
  const qc_handle* const h = reinterpret_cast<const qc_handle*>(buf);  // only compared with null
  qc_batch_in in{};
  in.joint_q = buf;
  const qc_torque_tangent_io io = valid_io();
  const char* const who = "qc_torque_tangent_batch";
  const auto msg = [who](const char* what) { return std::string(who) + what; };
  CHECK(check_torque_tangent_args(h, 1, &in, &io) == QC_OK, "the smallest valid call (one tangent in, written in place)");
  {
    qc_torque_tangent_io c = io;
    c.joint_q_tan = buf + 12;
    c.n_dir = 12;
    CHECK(check_torque_tangent_args(h, 4097, &in, &c) == QC_OK, "both tangents, K = 12");
    c.grf_tan = nullptr;
    CHECK(check_torque_tangent_args(h, 4097, &in, &c) == QC_OK, "joint_q_tan alone");
  }
  CHECK_FAILS(check_torque_tangent_args(nullptr, 1, &in, &io), msg(": null argument"), "no handle");
  CHECK_FAILS(check_torque_tangent_args(h, 1, nullptr, &io), msg(": null argument"), "no batch");
  CHECK_FAILS(check_torque_tangent_args(h, 1, &in, nullptr), msg(": null argument"), "no io");
  CHECK_FAILS(check_torque_tangent_args(nullptr, 0, &in, &io), msg(": null argument"), "no handle, n = 0");
  for (const size_t sz : {(size_t)0, sizeof(qc_torque_tangent_io) - 8, sizeof(qc_torque_tangent_io) + 8, sizeof(qc_tangent_io)}) {
    qc_torque_tangent_io c = io;
    c.struct_size = sz;
    char text[320];
    std::snprintf(text, sizeof text, "%s: qc_torque_tangent_io.struct_size is %zu, this library's qc_torque_tangent_io has %zu B (qc_default_torque_tangent sets it)",
                  who, sz, sizeof(qc_torque_tangent_io));
    CHECK_FAILS(check_torque_tangent_args(h, 1, &in, &c), text, "struct_size %zu", sz);
    CHECK_FAILS(check_torque_tangent_args(h, 0, &in, &c), text, "struct_size %zu, n = 0", sz);
  }
  {
    qc_torque_tangent_io c = io;
    c.n_dir = 0;
    CHECK_FAILS(check_torque_tangent_args(h, 1, &in, &c), msg(": n_dir must be >= 1"), "n_dir 0");
    CHECK_FAILS(check_torque_tangent_args(h, 0, &in, &c), msg(": n_dir must be >= 1"), "n_dir 0, n = 0");
  }
  {
    qc_torque_tangent_io c = io;
    c.joint_tau_tan = nullptr;
    CHECK_FAILS(check_torque_tangent_args(h, 1, &in, &c), msg(": no output requested (joint_tau_tan is NULL)"), "no output");
    CHECK_FAILS(check_torque_tangent_args(h, 0, &in, &c), msg(": no output requested (joint_tau_tan is NULL)"), "no output, n = 0");
  }
  {
    qc_torque_tangent_io c = io;
    c.grf_tan = nullptr;
    CHECK_FAILS(check_torque_tangent_args(h, 1, &in, &c), msg(": no tangent given (grf_tan and joint_q_tan are both NULL)"), "no tangent");
    CHECK_FAILS(check_torque_tangent_args(h, 0, &in, &c), msg(": no tangent given (grf_tan and joint_q_tan are both NULL)"), "no tangent, n = 0");
  }
  {
    qc_torque_tangent_io c = io;
    c.grf_body = nullptr;
    CHECK_FAILS(check_torque_tangent_args(h, 1, &in, &c), msg(": joint_tau_tan needs grf_body and status"), "no grf_body");
    c = io;
    c.status = nullptr;
    CHECK_FAILS(check_torque_tangent_args(h, 1, &in, &c), msg(": joint_tau_tan needs grf_body and status"), "no status");
    CHECK_FAILS(check_torque_tangent_args(h, 0, &in, &c), msg(": joint_tau_tan needs grf_body and status"), "no status, n = 0");
  }
  {
    qc_batch_in none{};
    none.feet = buf;  // (feet do not stand in for joint_q: the map is the joints')
    CHECK_FAILS(check_torque_tangent_args(h, 1, &none, &io), msg(": joint_q is required"), "no joint_q");
    CHECK(check_torque_tangent_args(h, 0, &none, &io) == QC_OK, "no joint_q, n = 0 asks for no array");
  }
  // one lane per (direction, robot, leg): the rows must fit a launch
  const size_t most = (size_t)0xFFFFFF * TORQUE_TANGENT_BLOCK / 4;
  CHECK(check_torque_tangent_args(h, most, &in, &io) == QC_OK, "the largest batch of one launch, K = 1");
  CHECK_FAILS(check_torque_tangent_args(h, most + 1, &in, &io), msg(": 4 * n * n_dir is beyond one launch"), "one robot more");
  {
    qc_torque_tangent_io c = io;
    c.n_dir = 16;
    CHECK(check_torque_tangent_args(h, (size_t)0xFFFFFF, &in, &c) == QC_OK, "the largest 4 n K, K = 16");
    CHECK_FAILS(check_torque_tangent_args(h, (size_t)0xFFFFFF + 1, &in, &c), msg(": 4 * n * n_dir is beyond one launch"), "one robot more at K = 16");
    c.n_dir = most;
    CHECK(check_torque_tangent_args(h, 1, &in, &c) == QC_OK, "one robot, the most directions");
    c.n_dir = most + 1;
    CHECK_FAILS(check_torque_tangent_args(h, 1, &in, &c), msg(": 4 * n * n_dir is beyond one launch"), "one direction more");
    c.n_dir = std::numeric_limits<size_t>::max();  // (a product that would wrap)
    CHECK_FAILS(check_torque_tangent_args(h, 3, &in, &c), msg(": 4 * n * n_dir is beyond one launch"), "n_dir = SIZE_MAX");
    CHECK_FAILS(check_torque_tangent_args(h, std::numeric_limits<size_t>::max() / 2, &in, &c), msg(": 4 * n * n_dir is beyond one launch"), "n and n_dir huge");
    CHECK(check_torque_tangent_args(h, 0, &in, &c) == QC_OK, "n = 0 launches nothing whatever n_dir is");
  }
  CHECK(sizeof(qc_torque_tangent_io) == 7 * 8, "the io record: struct_size, grf_body, status, n_dir, two tangents, one output");
  CHECK(sizeof(qc_tangent_io) == 17 * 8 && sizeof(qc_plant_tangent_io) == 20 * 8, "the other records keep their sizes");
}

static void constants() {
  qc_batch_in in{};
  in.joint_q = buf + 0; in.stance = bbuf; in.gait_phase = buf + 1; in.gait_duty = buf + 2;
  in.Rwb = buf + 20; in.feet = buf + 21;  // (not the kernel's business)
  qc_torque_tangent_io io{};
  io.grf_body = buf + 3; io.status = ibuf; io.n_dir = 7; io.grf_tan = buf + 4; io.joint_q_tan = buf + 5; io.joint_tau_tan = buf + 6;
  const TorqueTangentArgs a = torque_tangent_constants(&in, &io);
  CHECK(a.joint_q == buf + 0 && a.stance == bbuf && a.gait_phase == buf + 1 && a.gait_duty == buf + 2, "joint_q and the contact inputs of the batch");
  CHECK(a.grf_body == buf + 3 && a.status == ibuf && a.n_dir == 7 && a.grf_tan == buf + 4 && a.joint_q_tan == buf + 5 && a.joint_tau_tan == buf + 6, "the record's arrays and K");
  CHECK(sizeof(TorqueTangentArgs) == 10 * 8, "the kernarg layout is the flat one");
}

static void blocks() {
  CHECK(torque_tangent_blocks(1, 1) == 1 && torque_tangent_blocks(16, 1) == 1 && torque_tangent_blocks(17, 1) == 2, "one wave of 16 robots' legs per workgroup");
  CHECK(torque_tangent_blocks(6, 3) == 2 && torque_tangent_blocks(16, 12) == 12, "K multiplies the rows");
  const size_t cap = (size_t)TORQUE_TANGENT_MAX_BLOCKS * TORQUE_TANGENT_BLOCK / 4;
  CHECK(torque_tangent_blocks(cap, 1) == TORQUE_TANGENT_MAX_BLOCKS && torque_tangent_blocks(cap + 1, 1) == TORQUE_TANGENT_MAX_BLOCKS &&
            torque_tangent_blocks(cap / 4 + 1, 4) == TORQUE_TANGENT_MAX_BLOCKS && torque_tangent_blocks(cap - 16, 1) == TORQUE_TANGENT_MAX_BLOCKS - 1,
        "the grid cap: the waves stride beyond it");
}

int main() {
  arguments();
  constants();
  blocks();
  std::printf("torque tangent host logic ok (%ld checks)\n", g_checked);
  return 0;
}
