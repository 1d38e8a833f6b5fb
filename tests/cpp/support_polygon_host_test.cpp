// The device-free host logic of the support polygon's two entry points (quadruped_control_amd/csrc/qc_host.hpp,
// qc_support_polygon.hpp): check_support_polygon_args and check_support_polygon_adjoint_args through every refusal of
// qc_support_polygon_batch and qc_support_polygon_adjoint_batch and the accepted combinations of their optional arrays, and the
// adjacency table against the reference's map (trajectory.cpp:75-78).
// Host compiler only - links neither HIP nor the library; built with the address and undefined-behaviour sanitizers
// (__graft_entry__.build_host_test) and run by tests/test_support_polygon_cpu.py.  Prints the failing case and exits 1 on the
// first violated check.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "host_check.hpp"

using namespace qc;

static double buf[16];
static int32_t words[4];
static uint8_t bytes[4];
static qc_swing_state records[1];

static qc_batch_in valid_in() {
  qc_batch_in in{};
  in.feet = buf;
  in.gait_phase = buf;
  return in;
}

static void adjacency() {
  const char* const names[4] = {"RL", "FL", "RR", "FR"};
  // adjacent_leg_map_: name -> (first, second)
  const char* const ref[4][3] = {{"RL", "FL", "RR"}, {"FL", "FR", "RL"}, {"FR", "RR", "FL"}, {"RR", "RL", "FR"}};
  for (const auto& row : ref) {
    int l = -1;
    for (int k = 0; k < 4; k++)
      if (!std::strcmp(names[k], row[0])) l = k;
    CHECK(l >= 0 && !std::strcmp(names[SUPPORT_MINUS[l]], row[1]) && !std::strcmp(names[SUPPORT_PLUS[l]], row[2]), "the neighbours of %s", row[0]);
  }
  for (int l = 0; l < 4; l++) {
    CHECK(SUPPORT_MINUS[l] != l && SUPPORT_PLUS[l] != l && SUPPORT_MINUS[l] != SUPPORT_PLUS[l], "leg %d: two neighbours, neither itself", l);
    CHECK(SUPPORT_PLUS[SUPPORT_MINUS[l]] == l && SUPPORT_MINUS[SUPPORT_PLUS[l]] == l, "leg %d: the ring closes", l);
  }
  for (int k = 0; k + 1 < 4; k++)
    CHECK(std::strcmp(names[SUPPORT_SUM_ORDER[k]], names[SUPPORT_SUM_ORDER[k + 1]]) < 0, "the sum follows the order of the names (std::map), position %d", k);
}

template <class Io, class Check>
static void shared_refusals(const char* who, const qc_handle* h, const qc_batch_in& in, const Io& io, Check check) {
  const std::string w(who);
  const std::string null_arg = w + ": null argument";
  CHECK_FAILS(check(nullptr, 1, &in, &io), null_arg, "no handle");
  CHECK_FAILS(check(h, 1, nullptr, &io), null_arg, "no in");
  CHECK_FAILS(check(h, 1, &in, nullptr), null_arg, "no io");
  CHECK_FAILS(check(nullptr, 0, &in, &io), null_arg, "no handle, n = 0");
  {
    qc_batch_in b = in;
    b.gait_dt = buf;
    CHECK_FAILS(check(h, 1, &b, &io), w + ": gait_dt must be NULL (no clock is advanced: gait_phase is read as it is now)", "gait_dt given");
    CHECK_FAILS(check(h, 0, &b, &io), w + ": gait_dt must be NULL (no clock is advanced: gait_phase is read as it is now)", "gait_dt given, n = 0");
    b = in;
    b.swing_state = records;
    CHECK_FAILS(check(h, 1, &b, &io), w + ": swing_state must be NULL (nothing is planned here)", "swing_state given");
    const std::string refs = w + ": swing_pos and swing_vel must be NULL (the polygon reads the feet, not the swing references)";
    b = in;
    b.swing_pos = buf;
    CHECK_FAILS(check(h, 1, &b, &io), refs, "swing_pos given");
    b = in;
    b.swing_vel = buf;
    CHECK_FAILS(check(h, 1, &b, &io), refs, "swing_vel given");
  }
  {
    Io c = io;
    c.schedule = nullptr;
    CHECK_FAILS(check(h, 1, &in, &c), w + ": schedule is required (the widths of the ramps, [n][4][4] or one shared [4][4])", "no schedule");
    CHECK(check(h, 0, &in, &c) == QC_OK, "no schedule, n = 0 asks for no array");
  }
  {
    qc_batch_in b = in;
    b.gait_phase = nullptr;
    CHECK_FAILS(check(h, 1, &b, &io), w + ": gait_phase is required", "no gait_phase");
    b = in;
    b.feet = nullptr;
    CHECK_FAILS(check(h, 1, &b, &io), w + ": feet or joint_q is required", "neither feet nor joint_q");
    b.joint_q = buf;
    CHECK(check(h, 1, &b, &io) == QC_OK, "joint_q alone");
    b.feet = buf;
    CHECK(check(h, 1, &b, &io) == QC_OK, "feet and joint_q");
    b.stance = bytes; b.gait_duty = buf; b.Rwb_d = b.x_d = b.xdot = b.joint_qdot = buf;  // the mask's arrays; the rest is ignored
    CHECK(check(h, 4097, &b, &io) == QC_OK, "stance bytes, a duty per robot, arrays that are ignored");
  }
  {
    Io c = io;
    c.world = 1;
    const std::string text = w + ": world needs Rwb and x";
    CHECK_FAILS(check(h, 1, &in, &c), text, "world without Rwb and x");
    qc_batch_in b = in;
    b.Rwb = buf;
    CHECK_FAILS(check(h, 1, &b, &c), text, "world without x");
    b.Rwb = nullptr; b.x = buf;
    CHECK_FAILS(check(h, 1, &b, &c), text, "world without Rwb");
    b.Rwb = buf;
    CHECK(check(h, 1, &b, &c) == QC_OK, "world with Rwb and x");
    c.schedule_shared = 1;
    CHECK(check(h, 1, &b, &c) == QC_OK, "world, shared schedule");
  }
  const size_t most = (size_t)0xFFFFFF * SENSITIVITY_BLOCK;
  CHECK(check(h, most, &in, &io) == QC_OK, "the largest batch of one launch");
  CHECK_FAILS(check(h, most + 1, &in, &io), w + ": n is beyond one launch", "one robot more");
}

static void forward() {
  const qc_handle* const h = reinterpret_cast<const qc_handle*>(buf);  // only compared with null
  const qc_batch_in in = valid_in();
  qc_support_polygon_io io{};
  io.struct_size = sizeof(qc_support_polygon_io);
  io.schedule = buf;
  io.com_xy = buf;
  const auto check = [](const qc_handle* hh, size_t n, const qc_batch_in* b, const qc_support_polygon_io* c) { return check_support_polygon_args(hh, n, b, c); };
  CHECK(check(h, 1, &in, &io) == QC_OK, "feet, phases, a schedule -> com_xy");
  for (int k = 0; k < 3; k++) {
    qc_support_polygon_io c = io;
    c.com_xy = nullptr;
    if (k == 0) c.com_xy = buf;
    if (k == 1) c.weights = buf;
    if (k == 2) c.flags = words;
    CHECK(check(h, 1, &in, &c) == QC_OK, "output %d alone", k);
  }
  for (const size_t sz : {(size_t)0, sizeof(qc_support_polygon_io) - 8, sizeof(qc_support_polygon_io) + 8, sizeof(qc_support_polygon_adjoint_io)}) {
    qc_support_polygon_io c = io;
    c.struct_size = sz;
    char text[320];
    std::snprintf(text, sizeof text,
                  "qc_support_polygon_batch: qc_support_polygon_io.struct_size is %zu, this library's qc_support_polygon_io has %zu B (qc_default_support_polygon sets it)",
                  sz, sizeof(qc_support_polygon_io));
    CHECK_FAILS(check(h, 1, &in, &c), text, "struct_size %zu", sz);
    CHECK_FAILS(check(h, 0, &in, &c), text, "struct_size %zu, n = 0", sz);
  }
  {
    const char* const none = "qc_support_polygon_batch: no output requested (com_xy, weights, flags are all NULL)";
    qc_support_polygon_io c = io;
    c.com_xy = nullptr;
    CHECK_FAILS(check(h, 1, &in, &c), none, "no output");
    CHECK_FAILS(check(h, 0, &in, &c), none, "no output, n = 0");
  }
  shared_refusals("qc_support_polygon_batch", h, in, io, check);
  CHECK(sizeof(qc_support_polygon_io) == 6 * 8, "the io record: struct_size, schedule, two flags in one word, three outputs");
}

static void adjoint() {
  const qc_handle* const h = reinterpret_cast<const qc_handle*>(buf);
  const qc_batch_in in = valid_in();
  qc_support_polygon_adjoint_io io{};
  io.struct_size = sizeof(qc_support_polygon_adjoint_io);
  io.schedule = buf;
  io.com_xy_bar = buf;
  io.feet_bar = buf;
  const auto check = [](const qc_handle* hh, size_t n, const qc_batch_in* b, const qc_support_polygon_adjoint_io* c) {
    return check_support_polygon_adjoint_args(hh, n, b, c);
  };
  CHECK(check(h, 1, &in, &io) == QC_OK, "feet, phases, a schedule, the cotangent -> feet_bar");
  for (int k = 0; k < 6; k++) {
    qc_support_polygon_adjoint_io c = io;
    c.feet_bar = nullptr;
    if (k == 0) c.feet_bar = buf;
    if (k == 1) c.Rwb_bar = buf;
    if (k == 2) c.x_bar = buf;
    if (k == 3) c.phase_bar = buf;
    if (k == 4) c.schedule_bar = buf;
    if (k == 5) c.flags = words;
    CHECK(check(h, 1, &in, &c) == QC_OK, "output %d alone", k);
  }
  {
    qc_support_polygon_adjoint_io c = io;
    c.feet_bar_in = c.feet_bar;  // in place
    c.Rwb_bar_in = c.x_bar_in = c.phase_bar_in = c.schedule_bar_in = buf;
    c.Rwb_bar = c.x_bar = c.phase_bar = c.schedule_bar = buf;
    CHECK(check(h, 1, &in, &c) == QC_OK, "every accumulator, every output");
  }
  for (const size_t sz : {(size_t)0, sizeof(qc_support_polygon_adjoint_io) - 8, sizeof(qc_support_polygon_adjoint_io) + 8, sizeof(qc_support_polygon_io)}) {
    qc_support_polygon_adjoint_io c = io;
    c.struct_size = sz;
    char text[360];
    std::snprintf(text, sizeof text,
                  "qc_support_polygon_adjoint_batch: qc_support_polygon_adjoint_io.struct_size is %zu, this library's qc_support_polygon_adjoint_io has %zu B "
                  "(qc_default_support_polygon_adjoint sets it)",
                  sz, sizeof(qc_support_polygon_adjoint_io));
    CHECK_FAILS(check(h, 1, &in, &c), text, "struct_size %zu", sz);
  }
  {
    const char* const none = "qc_support_polygon_adjoint_batch: no output requested (feet_bar, Rwb_bar, x_bar, phase_bar, schedule_bar, flags are all NULL)";
    qc_support_polygon_adjoint_io c = io;
    c.feet_bar = nullptr;
    CHECK_FAILS(check(h, 1, &in, &c), none, "no output");
    CHECK_FAILS(check(h, 0, &in, &c), none, "no output, n = 0");
    c = io;
    c.com_xy_bar = nullptr;
    CHECK_FAILS(check(h, 1, &in, &c), "qc_support_polygon_adjoint_batch: com_xy_bar is required", "no cotangent");
    CHECK(check(h, 0, &in, &c) == QC_OK, "no cotangent, n = 0 asks for no array");
  }
  shared_refusals("qc_support_polygon_adjoint_batch", h, in, io, check);
  CHECK(sizeof(qc_support_polygon_adjoint_io) == 15 * 8, "the io record: struct_size, schedule, two flags, the cotangent, five accumulators, six outputs");
  CHECK(sizeof(qc_swing_reference_adjoint_io) == 20 * 8 && sizeof(qc_batch_in) == 18 * 8, "the neighbours keep their size");
}

int main() {
  adjacency();
  forward();
  adjoint();
  std::printf("support polygon host logic ok (%ld checks)\n", g_checked);
  return 0;
}
