// The device-free host logic of the COM reference's two entry points (quadruped_control_amd/csrc/qc_host.hpp, qc_com_reference.hpp):
// check_com_reference_args and check_com_reference_adjoint_args through every refusal of qc_com_reference_batch and
// qc_com_reference_adjoint_batch and the accepted combinations of their optional arrays, the launch geometry of the summing reverse
// pass and the constants its documented order of additions rests on.
// Host compiler only - links neither HIP nor the library; built with the address and undefined-behaviour sanitizers
// (__graft_entry__.build_host_test) and run by tests/test_com_reference_cpu.py.  Prints the failing case and exits 1 on the first
// violated check.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
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
  in.Rwb = buf;
  in.x = buf;
  return in;
}

template <class Io, class Check>
static void shared_refusals(const char* who, const qc_handle* h, const qc_batch_in& in, const Io& io, Check check) {
  const std::string w(who);
  const std::string null_arg = w + ": null argument";
  CHECK_FAILS(check(nullptr, 1, &in, &io), null_arg, "no handle");
  CHECK_FAILS(check(h, 1, nullptr, &io), null_arg, "no in");
  CHECK_FAILS(check(h, 1, &in, nullptr), null_arg, "no io");
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
    c.mode = 2;
    CHECK_FAILS(check(h, 1, &in, &c), w + ": mode must be QC_COM_REPLACE or QC_COM_OFFSET", "mode 2");
    c.mode = -1;
    CHECK_FAILS(check(h, 0, &in, &c), w + ": mode must be QC_COM_REPLACE or QC_COM_OFFSET", "mode -1, n = 0");
    c.mode = QC_COM_OFFSET;
    CHECK(check(h, 1, &in, &c) == QC_OK, "offset mode");
    c.gain = 0.0;
    CHECK(check(h, 1, &in, &c) == QC_OK, "gain 0");
    c.gain = -2.5;
    CHECK(check(h, 1, &in, &c) == QC_OK, "a negative gain");
    c.gain = std::numeric_limits<double>::infinity();
    CHECK_FAILS(check(h, 1, &in, &c), w + ": gain must be finite", "gain inf");
    c.gain = std::nan("");
    c.mode = QC_COM_REPLACE;
    CHECK_FAILS(check(h, 1, &in, &c), w + ": gain must be finite", "gain NaN (replace mode does not read it, the check does)");
  }
  {
    Io c = io;
    c.schedule = nullptr;
    CHECK_FAILS(check(h, 1, &in, &c), w + ": schedule is required (the widths of the ramps, [n][4][4] or one shared [4][4])", "no schedule");
    CHECK(check(h, 0, &in, &c) == QC_OK, "no schedule, n = 0 asks for no array");
    c = io;
    c.schedule_shared = 1;
    CHECK(check(h, 1, &in, &c) == QC_OK, "shared schedule");
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
    b.stance = bytes; b.gait_duty = buf; b.Rwb_d = b.x_d = b.xdot = b.joint_qdot = buf;  // the mask's arrays; the rest is ignored
    CHECK(check(h, 4097, &b, &io) == QC_OK, "stance bytes, a duty per robot, arrays that are ignored");
    const std::string pose = w + ": Rwb and x are required (the polygon is that of Rwb p + x)";
    b = in;
    b.Rwb = nullptr;
    CHECK_FAILS(check(h, 1, &b, &io), pose, "no Rwb");
    b = in;
    b.x = nullptr;
    CHECK_FAILS(check(h, 1, &b, &io), pose, "no x");
    CHECK(check(h, 0, &b, &io) == QC_OK, "no x, n = 0 asks for no array");
  }
  const size_t most = (size_t)0xFFFFFF * SENSITIVITY_BLOCK;
  CHECK(check(h, most, &in, &io) == QC_OK, "the largest batch of one launch");
  CHECK_FAILS(check(h, most + 1, &in, &io), w + ": n is beyond one launch", "one robot more");
}

static void forward() {
  const qc_handle* const h = reinterpret_cast<const qc_handle*>(buf);  // only compared with null
  const qc_batch_in in = valid_in();
  qc_com_reference_io io{};
  io.struct_size = sizeof(qc_com_reference_io);
  io.gain = 1.0;
  io.schedule = buf;
  io.x_d_in = buf;
  io.x_d_out = buf;  // in place
  const auto check = [](const qc_handle* hh, size_t n, const qc_batch_in* b, const qc_com_reference_io* c) { return check_com_reference_args(hh, n, b, c); };
  CHECK(check(h, 1, &in, &io) == QC_OK, "feet, phases, pose, a schedule, x_d in place");
  {
    qc_com_reference_io c = io;
    c.com_xy = buf;
    c.flags = words;
    CHECK(check(h, 1, &in, &c) == QC_OK, "every output");
    c = io;
    c.x_d_out = nullptr;
    c.com_xy = buf;
    CHECK_FAILS(check(h, 1, &in, &c), "qc_com_reference_batch: x_d_out is required", "no x_d_out");
    CHECK_FAILS(check(h, 0, &in, &c), "qc_com_reference_batch: x_d_out is required", "no x_d_out, n = 0");
    c = io;
    c.x_d_in = nullptr;
    CHECK_FAILS(check(h, 1, &in, &c), "qc_com_reference_batch: x_d_in is required", "no x_d_in");
    CHECK(check(h, 0, &in, &c) == QC_OK, "no x_d_in, n = 0 asks for no array");
  }
  for (const size_t sz : {(size_t)0, sizeof(qc_com_reference_io) - 8, sizeof(qc_com_reference_io) + 8, sizeof(qc_com_reference_adjoint_io)}) {
    qc_com_reference_io c = io;
    c.struct_size = sz;
    char text[320];
    std::snprintf(text, sizeof text,
                  "qc_com_reference_batch: qc_com_reference_io.struct_size is %zu, this library's qc_com_reference_io has %zu B (qc_default_com_reference sets it)",
                  sz, sizeof(qc_com_reference_io));
    CHECK_FAILS(check(h, 1, &in, &c), text, "struct_size %zu", sz);
    CHECK_FAILS(check(h, 0, &in, &c), text, "struct_size %zu, n = 0", sz);
  }
  shared_refusals("qc_com_reference_batch", h, in, io, check);
  CHECK(sizeof(qc_com_reference_io) == 8 * 8, "the io record: struct_size, schedule, two words in one, gain, x_d_in, three outputs");
}

static void adjoint() {
  const qc_handle* const h = reinterpret_cast<const qc_handle*>(buf);
  const qc_batch_in in = valid_in();
  qc_com_reference_adjoint_io io{};
  io.struct_size = sizeof(qc_com_reference_adjoint_io);
  io.gain = 1.0;
  io.schedule = buf;
  io.x_d_out_bar = buf;
  io.x_d_in_bar = buf;  // in place
  const auto check = [](const qc_handle* hh, size_t n, const qc_batch_in* b, const qc_com_reference_adjoint_io* c) {
    return check_com_reference_adjoint_args(hh, n, b, c);
  };
  CHECK(check(h, 1, &in, &io) == QC_OK, "the cotangent -> x_d_in_bar over it");
  for (int k = 0; k < 8; k++) {
    qc_com_reference_adjoint_io c = io;
    c.x_d_in_bar = nullptr;
    if (k == 0) c.x_d_in_bar = buf;
    if (k == 1) c.feet_bar = buf;
    if (k == 2) c.Rwb_bar = buf;
    if (k == 3) c.x_bar = buf;
    if (k == 4) c.phase_bar = buf;
    if (k == 5) c.schedule_bar = buf;
    if (k == 6) c.schedule_bar_sum = buf;
    if (k == 7) c.flags = words;
    CHECK(check(h, 1, &in, &c) == QC_OK, "output %d alone", k);
  }
  {
    qc_com_reference_adjoint_io c = io;
    c.feet_bar_in = c.Rwb_bar_in = c.x_bar_in = c.phase_bar_in = c.schedule_bar_in = buf;
    c.feet_bar = c.Rwb_bar = c.x_bar = c.phase_bar = c.schedule_bar = c.schedule_bar_sum = buf;
    CHECK(check(h, 1, &in, &c) == QC_OK, "every accumulator, every output, the sum");
  }
  for (const size_t sz : {(size_t)0, sizeof(qc_com_reference_adjoint_io) - 8, sizeof(qc_com_reference_adjoint_io) + 8, sizeof(qc_com_reference_io)}) {
    qc_com_reference_adjoint_io c = io;
    c.struct_size = sz;
    char text[360];
    std::snprintf(text, sizeof text,
                  "qc_com_reference_adjoint_batch: qc_com_reference_adjoint_io.struct_size is %zu, this library's qc_com_reference_adjoint_io has %zu B "
                  "(qc_default_com_reference_adjoint sets it)",
                  sz, sizeof(qc_com_reference_adjoint_io));
    CHECK_FAILS(check(h, 1, &in, &c), text, "struct_size %zu", sz);
  }
  {
    const char* const none =
        "qc_com_reference_adjoint_batch: no output requested (x_d_in_bar, feet_bar, Rwb_bar, x_bar, phase_bar, schedule_bar, schedule_bar_sum, flags are all NULL)";
    qc_com_reference_adjoint_io c = io;
    c.x_d_in_bar = nullptr;
    CHECK_FAILS(check(h, 1, &in, &c), none, "no output");
    CHECK_FAILS(check(h, 0, &in, &c), none, "no output, n = 0");
    c = io;
    c.x_d_out_bar = nullptr;
    CHECK_FAILS(check(h, 1, &in, &c), "qc_com_reference_adjoint_batch: x_d_out_bar is required", "no cotangent");
    CHECK(check(h, 0, &in, &c) == QC_OK, "no cotangent, n = 0 asks for no array");
  }
  shared_refusals("qc_com_reference_adjoint_batch", h, in, io, check);
  CHECK(sizeof(qc_com_reference_adjoint_io) == 18 * 8, "the io record: struct_size, schedule, two words, gain, the cotangent, five accumulators, eight outputs");
  CHECK(sizeof(qc_support_polygon_adjoint_io) == 15 * 8 && sizeof(qc_batch_in) == 18 * 8, "the neighbours keep their size");
}

static void geometry() {
  CHECK(COM_REPLACE == QC_COM_REPLACE && COM_OFFSET == QC_COM_OFFSET, "the modes of the kernels are the header's");
  CHECK(SENSITIVITY_BLOCK == 64 && COM_SUM_MAX_BLOCKS == 1024 && COM_SUM_GROUPS == 16 && COM_SUM_FINISH_BLOCK == 256,
        "the constants of the documented order of additions (include/qc_balance.h)");
  CHECK(COM_SUM_STRIDE % 2 == 1 && COM_SUM_STRIDE >= 16, "an odd stride that holds the 16 numbers");
  CHECK(com_reference_blocks(1, true) == 1 && com_reference_blocks(64, true) == 1 && com_reference_blocks(65, true) == 2, "one wave per workgroup");
  CHECK(com_reference_blocks(65536, true) == 1024 && com_reference_blocks(65537, true) == 1024, "the sum's grid stops at the partials of the buffer");
  CHECK(com_reference_blocks(65537, false) == 1025 && com_reference_blocks((size_t)1 << 30, false) == (unsigned)SENSITIVITY_MAX_BLOCKS,
        "without the sum: the polygon's geometry");
}

int main() {
  forward();
  adjoint();
  geometry();
  std::printf("com reference host logic ok (%ld checks)\n", g_checked);
  return 0;
}
