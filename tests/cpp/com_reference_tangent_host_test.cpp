// The device-free host logic of the COM reference's forward mode (quadruped_control_amd/csrc/qc_host.hpp):
// check_com_reference_tangent_args through every refusal of qc_com_reference_tangent_batch - qc_com_reference_adjoint_batch's about
// `in`, the mode, the gain and the schedule, in its words, and the tangent's own -, com_reference_tangent_constants - the kernel's
// arguments - and com_reference_tangent_dirs.  Host compiler only - links neither HIP nor the library; built with the address and
// undefined-behaviour sanitizers (__graft_entry__.build_host_test) and run by tests/test_com_reference_tangent_cpu.py.  Prints the
// failing case and exits 1 on the first violated check.
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <string>

#include "host_check.hpp"

using namespace qc;

static double buf[40];
static int32_t ibuf[4];
static uint8_t bbuf[4];
static qc_swing_state records[1];

static qc_batch_in valid_in() {
  qc_batch_in in{};
  in.Rwb = buf; in.x = buf + 1; in.feet = buf + 2; in.gait_phase = buf + 3;
  return in;
}

static qc_com_reference_tangent_io valid_io() {
  qc_com_reference_tangent_io io{};
  io.struct_size = sizeof(qc_com_reference_tangent_io);
  io.schedule = buf + 4;
  io.mode = COM_REPLACE;
  io.gain = 1.0;
  io.n_dir = 1;
  io.schedule_tan = buf + 5;
  io.x_d_out_tan = buf + 6;
  return io;
}

static void arguments() {
  const qc_handle* const h = reinterpret_cast<const qc_handle*>(buf);  // only compared with null
  const qc_batch_in in = valid_in();
  const qc_com_reference_tangent_io io = valid_io();
  const char* const who = "qc_com_reference_tangent_batch";
  const auto msg = [who](const char* what) { return std::string(who) + what; };
  CHECK(check_com_reference_tangent_args(h, 1, &in, &io) == QC_OK, "the smallest valid call");
  {
    qc_com_reference_tangent_io c = io;
    qc_batch_in b = in;
    b.joint_q = buf + 7; b.stance = bbuf; b.gait_duty = buf + 8;
    c.x_d_in_tan = c.x_d_out_tan = buf + 9;  // in place
    c.feet_tan = buf + 10; c.joint_q_tan = buf + 11; c.Rwb_rot_tan = buf + 12; c.x_tan = buf + 13; c.phase_tan = buf + 14;
    c.com_xy_tan = buf + 15; c.flags = ibuf; c.n_dir = 16; c.mode = COM_OFFSET; c.gain = -0.5; c.schedule_shared = 1;
    CHECK(check_com_reference_tangent_args(h, 4097, &b, &c) == QC_OK, "every tangent, every output, K = 16, a shared schedule");
    c.x_d_out_tan = c.com_xy_tan = nullptr;
    CHECK(check_com_reference_tangent_args(h, 4097, &b, &c) == QC_OK, "the flags alone");
    CHECK(com_reference_tangent_dirs(&c) == 1, "the flags alone walk one direction");
  }
  for (int k = 0; k < 6; k++) {  // each tangent alone (joint_q_tan: below)
    qc_com_reference_tangent_io c = io;
    c.schedule_tan = nullptr;
    const double** const slot[6] = {&c.x_d_in_tan, &c.feet_tan, &c.Rwb_rot_tan, &c.x_tan, &c.phase_tan, &c.schedule_tan};
    *slot[k] = buf + 16;
    CHECK(check_com_reference_tangent_args(h, 1, &in, &c) == QC_OK, "tangent %d alone", k);
  }
  for (int k = 0; k < 3; k++) {  // each output alone
    qc_com_reference_tangent_io c = io;
    c.x_d_out_tan = nullptr;
    if (k == 0) c.x_d_out_tan = buf + 17;
    if (k == 1) c.com_xy_tan = buf + 17;
    if (k == 2) c.flags = ibuf;
    CHECK(check_com_reference_tangent_args(h, 1, &in, &c) == QC_OK, "output %d alone", k);
  }
  CHECK_FAILS(check_com_reference_tangent_args(nullptr, 1, &in, &io), msg(": null argument"), "no handle");
  CHECK_FAILS(check_com_reference_tangent_args(h, 1, nullptr, &io), msg(": null argument"), "no batch");
  CHECK_FAILS(check_com_reference_tangent_args(h, 1, &in, nullptr), msg(": null argument"), "no io");
  for (const size_t sz : {(size_t)0, sizeof(qc_com_reference_tangent_io) - 8, sizeof(qc_com_reference_tangent_io) + 8}) {
    qc_com_reference_tangent_io c = io;
    c.struct_size = sz;
    char text[360];
    std::snprintf(text, sizeof text,
                  "%s: qc_com_reference_tangent_io.struct_size is %zu, this library's qc_com_reference_tangent_io has %zu B (qc_default_com_reference_tangent sets it)",
                  who, sz, sizeof(qc_com_reference_tangent_io));
    CHECK_FAILS(check_com_reference_tangent_args(h, 1, &in, &c), text, "struct_size %zu", sz);
    CHECK_FAILS(check_com_reference_tangent_args(h, 0, &in, &c), text, "struct_size %zu, n = 0", sz);
  }
  {  // what the adjoint refuses about `in`, first and in its words
    qc_batch_in c = in;
    c.gait_dt = buf;
    CHECK_FAILS(check_com_reference_tangent_args(h, 1, &c, &io), msg(": gait_dt must be NULL (no clock is advanced: gait_phase is read as it is now)"), "gait_dt");
    c = in;
    c.swing_state = records;
    CHECK_FAILS(check_com_reference_tangent_args(h, 1, &c, &io), msg(": swing_state must be NULL (nothing is planned here)"), "swing_state");
    for (int k = 0; k < 2; k++) {
      c = in;
      (k == 0 ? c.swing_pos : c.swing_vel) = buf;
      CHECK_FAILS(check_com_reference_tangent_args(h, 1, &c, &io), msg(": swing_pos and swing_vel must be NULL (the polygon reads the feet, not the swing references)"),
                  "swing reference %d", k);
    }
  }
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  {
    qc_com_reference_tangent_io c = io;
    c.mode = 2;
    CHECK_FAILS(check_com_reference_tangent_args(h, 1, &in, &c), msg(": mode must be QC_COM_REPLACE or QC_COM_OFFSET"), "an unknown mode");
    for (const double bad : {inf, -inf, nan}) {
      c = io;
      c.gain = bad;
      CHECK_FAILS(check_com_reference_tangent_args(h, 1, &in, &c), msg(": gain must be finite"), "gain %g", bad);
    }
    c = io;
    c.n_dir = 0;
    CHECK_FAILS(check_com_reference_tangent_args(h, 1, &in, &c), msg(": n_dir must be >= 1"), "n_dir 0");
    CHECK_FAILS(check_com_reference_tangent_args(h, 0, &in, &c), msg(": n_dir must be >= 1"), "n_dir 0, n = 0");
    c = io;
    c.schedule_tan = nullptr;
    const std::string none = msg(": no tangent given (x_d_in_tan, feet_tan, joint_q_tan, Rwb_rot_tan, x_tan, phase_tan, schedule_tan are all NULL)");
    CHECK_FAILS(check_com_reference_tangent_args(h, 1, &in, &c), none, "no tangent");
    CHECK_FAILS(check_com_reference_tangent_args(h, 0, &in, &c), none, "no tangent, n = 0");
    c = io;
    c.x_d_out_tan = nullptr;
    const std::string out = msg(": no output requested (x_d_out_tan, com_xy_tan, flags are all NULL)");
    CHECK_FAILS(check_com_reference_tangent_args(h, 1, &in, &c), out, "no output");
    CHECK_FAILS(check_com_reference_tangent_args(h, 0, &in, &c), out, "no output, n = 0");
    c = io;
    c.joint_q_tan = buf + 18;
    CHECK_FAILS(check_com_reference_tangent_args(h, 1, &in, &c), msg(": joint_q_tan needs in->joint_q"), "joint_q_tan without joint_q");
    qc_batch_in b = in;
    b.feet = nullptr; b.joint_q = buf + 7;
    CHECK(check_com_reference_tangent_args(h, 1, &b, &c) == QC_OK, "joint_q_tan with joint_q");
  }
  {
    qc_com_reference_tangent_io c = io;
    c.schedule = nullptr;
    CHECK_FAILS(check_com_reference_tangent_args(h, 1, &in, &c), msg(": schedule is required (the widths of the ramps, [n][4][4] or one shared [4][4])"), "no schedule");
    CHECK(check_com_reference_tangent_args(h, 0, &in, &c) == QC_OK, "n = 0 needs no schedule");
    qc_batch_in b = in;
    b.gait_phase = nullptr;
    CHECK_FAILS(check_com_reference_tangent_args(h, 1, &b, &io), msg(": gait_phase is required"), "no gait_phase");
    b = in;
    b.feet = nullptr;
    CHECK_FAILS(check_com_reference_tangent_args(h, 1, &b, &io), msg(": feet or joint_q is required"), "no feet");
    for (int k = 0; k < 2; k++) {
      b = in;
      (k == 0 ? b.Rwb : b.x) = nullptr;
      CHECK_FAILS(check_com_reference_tangent_args(h, 1, &b, &io), msg(": Rwb and x are required (the polygon is that of Rwb p + x)"), "missing pose array %d", k);
    }
  }
  {
    const size_t cap = (size_t)0xFFFFFF * (size_t)COMMAND_TANGENT_BLOCK;
    qc_com_reference_tangent_io c = io;
    CHECK(check_com_reference_tangent_args(h, cap, &in, &c) == QC_OK, "n at the launch bound, K = 1");
    CHECK_FAILS(check_com_reference_tangent_args(h, cap + 1, &in, &c), msg(": n is beyond one launch"), "n one past the bound");
    c.n_dir = 2;
    CHECK_FAILS(check_com_reference_tangent_args(h, cap, &in, &c), msg(": n * n_dir is beyond one launch"), "n at the bound, K = 2");
    c.n_dir = std::numeric_limits<size_t>::max();
    CHECK_FAILS(check_com_reference_tangent_args(h, 2, &in, &c), msg(": n * n_dir is beyond one launch"), "a product that would wrap");
  }
}

static void packing() {
  qc_batch_in in = valid_in();
  in.stance = bbuf; in.gait_duty = buf + 8;
  qc_com_reference_tangent_io io = valid_io();
  io.n_dir = 7; io.mode = COM_OFFSET; io.gain = 0.25; io.schedule_shared = 1; io.flags = ibuf; io.x_tan = buf + 19; io.com_xy_tan = buf + 20;
  const ComReferenceTangentArgs a = com_reference_tangent_constants(&in, &io);
  CHECK(a.feet == in.feet && !a.joint_q && a.gait_phase == in.gait_phase && a.stance == bbuf && a.gait_duty == in.gait_duty && a.Rwb == in.Rwb && a.x == in.x &&
            a.schedule == io.schedule && a.shared == 1,
        "what the forward call reads, world mode");
  CHECK(a.mode == COM_OFFSET && a.gain == 0.25 && a.n_dir == 7, "the mode, the gain and K");
  CHECK(!a.x_d_in_tan && !a.feet_tan && !a.joint_q_tan && !a.Rwb_rot_tan && a.x_tan == io.x_tan && !a.phase_tan && a.schedule_tan == io.schedule_tan, "the tangents");
  CHECK(a.x_d_out_tan == io.x_d_out_tan && a.com_xy_tan == io.com_xy_tan && a.flags == ibuf, "the outputs");
}

int main() {
  arguments();
  packing();
  std::printf("com reference tangent host logic ok\n");
  return 0;
}
