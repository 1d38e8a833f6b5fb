// The device-free host logic of the commander step's forward mode (quadruped_control_amd/csrc/qc_host.hpp):
// check_commander_step_tangent_args through every refusal of qc_commander_step_tangent_batch, commander_step_tangent_constants - the
// kernel's arguments -, commander_step_tangent_dirs and command_tangent_blocks at, and one past, the grid cap.  Host compiler only -
// links neither HIP nor the library; built with the address and undefined-behaviour sanitizers (__graft_entry__.build_host_test) and
// run by tests/test_commander_tangent_cpu.py.  Prints the failing case and exits 1 on the first violated check.
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
static qc_commander_state records[1];

static qc_batch_in valid_in() {
  qc_batch_in in{};
  in.Rwb = buf; in.x = buf + 1;
  return in;
}

static qc_command_in valid_cmd() {
  qc_command_in c{};
  c.struct_size = sizeof(qc_command_in);
  c.twist = buf + 2; c.fresh = bbuf;
  c.stand_height = 0.26; c.stand_tol = 0.005; c.cmd_dt = 0.001;
  return c;
}

static qc_commander_step_tangent_io valid_io() {
  qc_commander_step_tangent_io io{};
  io.struct_size = sizeof(qc_commander_step_tangent_io);
  io.state_before = records;
  io.n_dir = 1;
  io.twist_tan = buf + 3;
  io.x_d_tan = buf + 4;
  return io;
}

static void arguments() {
  const qc_handle* const h = reinterpret_cast<const qc_handle*>(buf);  // only compared with null
  const qc_batch_in in = valid_in();
  const qc_command_in cmd = valid_cmd();
  const qc_commander_step_tangent_io io = valid_io();
  const char* const who = "qc_commander_step_tangent_batch";
  const auto msg = [who](const char* what) { return std::string(who) + what; };
  CHECK(check_commander_step_tangent_args(h, 1, &in, &cmd, &io) == QC_OK, "the smallest valid call");
  {
    qc_commander_step_tangent_io c = io;
    c.Vb_tan = buf + 5; c.Rwb_rot_tan = buf + 6; c.x_tan = buf + 7;
    c.Rwb_d_rot_prev_tan = c.Rwb_d_rot_tan = buf + 8;  // in place: a rollout carries the record's tangents
    c.x_d_prev_tan = c.x_d_tan = buf + 9; c.xdot_d_prev_tan = c.xdot_d_tan = buf + 10; c.w_d_prev_tan = c.w_d_tan = buf + 11;
    c.Vb_next_tan = buf + 5; c.flags = ibuf; c.n_dir = 12;
    CHECK(check_commander_step_tangent_args(h, 4097, &in, &cmd, &c) == QC_OK, "every tangent, every output in place, K = 12");
    c.Rwb_d_rot_tan = c.x_d_tan = c.xdot_d_tan = c.w_d_tan = c.Vb_next_tan = nullptr;
    CHECK(check_commander_step_tangent_args(h, 4097, &in, &cmd, &c) == QC_OK, "the flags alone");
    CHECK(commander_step_tangent_dirs(&c) == 1, "the flags alone walk one direction");
  }
  for (int k = 0; k < 8; k++) {  // each tangent alone
    qc_commander_step_tangent_io c = io;
    c.twist_tan = nullptr;
    const double** const slot[8] = {&c.twist_tan, &c.Vb_tan, &c.Rwb_rot_tan, &c.x_tan, &c.Rwb_d_rot_prev_tan, &c.x_d_prev_tan, &c.xdot_d_prev_tan, &c.w_d_prev_tan};
    *slot[k] = buf + 12;
    CHECK(check_commander_step_tangent_args(h, 1, &in, &cmd, &c) == QC_OK, "tangent %d alone", k);
  }
  for (int k = 0; k < 6; k++) {  // each output alone
    qc_commander_step_tangent_io c = io;
    c.x_d_tan = nullptr;
    if (k == 5) c.flags = ibuf;
    else {
      double** const slot[5] = {&c.Rwb_d_rot_tan, &c.x_d_tan, &c.xdot_d_tan, &c.w_d_tan, &c.Vb_next_tan};
      *slot[k] = buf + 13;
    }
    CHECK(check_commander_step_tangent_args(h, 1, &in, &cmd, &c) == QC_OK, "output %d alone", k);
  }
  CHECK_FAILS(check_commander_step_tangent_args(nullptr, 1, &in, &cmd, &io), msg(": null argument"), "no handle");
  CHECK_FAILS(check_commander_step_tangent_args(h, 1, nullptr, &cmd, &io), msg(": null argument"), "no batch");
  CHECK_FAILS(check_commander_step_tangent_args(h, 1, &in, nullptr, &io), msg(": null argument"), "no command");
  CHECK_FAILS(check_commander_step_tangent_args(h, 1, &in, &cmd, nullptr), msg(": null argument"), "no io");
  CHECK_FAILS(check_commander_step_tangent_args(nullptr, 0, &in, &cmd, &io), msg(": null argument"), "no handle, n = 0");
  for (const size_t sz : {(size_t)0, sizeof(qc_commander_step_tangent_io) - 8, sizeof(qc_commander_step_tangent_io) + 8}) {
    qc_commander_step_tangent_io c = io;
    c.struct_size = sz;
    char text[360];
    std::snprintf(text, sizeof text,
                  "%s: qc_commander_step_tangent_io.struct_size is %zu, this library's qc_commander_step_tangent_io has %zu B (qc_default_commander_step_tangent sets it)",
                  who, sz, sizeof(qc_commander_step_tangent_io));
    CHECK_FAILS(check_commander_step_tangent_args(h, 1, &in, &cmd, &c), text, "struct_size %zu", sz);
    CHECK_FAILS(check_commander_step_tangent_args(h, 0, &in, &cmd, &c), text, "struct_size %zu, n = 0", sz);
  }
  {
    qc_command_in c = cmd;
    c.struct_size = 8;
    char text[360];
    std::snprintf(text, sizeof text, "%s: qc_command_in.struct_size is %zu, this library's qc_command_in has %zu B (qc_default_command sets it)", who, (size_t)8,
                  sizeof(qc_command_in));
    CHECK_FAILS(check_commander_step_tangent_args(h, 1, &in, &c, &io), text, "the command's struct_size");
  }
  {
    qc_commander_step_tangent_io c = io;
    c.n_dir = 0;
    CHECK_FAILS(check_commander_step_tangent_args(h, 1, &in, &cmd, &c), msg(": n_dir must be >= 1"), "n_dir 0");
    CHECK_FAILS(check_commander_step_tangent_args(h, 0, &in, &cmd, &c), msg(": n_dir must be >= 1"), "n_dir 0, n = 0");
  }
  {
    const std::string none =
        msg(": no tangent given (twist_tan, Vb_tan, Rwb_rot_tan, x_tan, Rwb_d_rot_prev_tan, x_d_prev_tan, xdot_d_prev_tan, w_d_prev_tan are all NULL)");
    qc_commander_step_tangent_io c = io;
    c.twist_tan = nullptr;
    CHECK_FAILS(check_commander_step_tangent_args(h, 1, &in, &cmd, &c), none, "no tangent");
    CHECK_FAILS(check_commander_step_tangent_args(h, 0, &in, &cmd, &c), none, "no tangent, n = 0");
  }
  {
    const std::string none = msg(": no output requested (Rwb_d_rot_tan, x_d_tan, xdot_d_tan, w_d_tan, Vb_next_tan, flags are all NULL)");
    qc_commander_step_tangent_io c = io;
    c.x_d_tan = nullptr;
    CHECK_FAILS(check_commander_step_tangent_args(h, 1, &in, &cmd, &c), none, "no output");
    CHECK_FAILS(check_commander_step_tangent_args(h, 0, &in, &cmd, &c), none, "no output, n = 0");
  }
  {
    qc_command_in c = cmd;
    c.twist = nullptr; c.fresh = nullptr;
    CHECK_FAILS(check_commander_step_tangent_args(h, 1, &in, &c, &io), msg(": twist_tan needs qc_command_in.twist"), "twist_tan without twist");
    qc_commander_step_tangent_io held = io;
    held.twist_tan = nullptr; held.Vb_tan = buf + 5;
    CHECK(check_commander_step_tangent_args(h, 1, &in, &c, &held) == QC_OK, "no command at all: the held one's tangent");
    c.fresh = bbuf;
    CHECK_FAILS(check_commander_step_tangent_args(h, 1, &in, &c, &held), msg(": qc_command_in.fresh needs twist"), "fresh without twist");
  }
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  for (int k = 0; k < 3; k++)
    for (const double bad : {inf, -inf, nan}) {
      qc_command_in c = cmd;
      (k == 0 ? c.stand_height : k == 1 ? c.stand_tol : c.cmd_dt) = bad;
      CHECK_FAILS(check_commander_step_tangent_args(h, 1, &in, &c, &io), msg(": stand_height, stand_tol (>= 0) and cmd_dt must be finite"), "scalar %d = %g", k, bad);
    }
  {
    qc_commander_step_tangent_io c = io;
    c.state_before = nullptr;
    CHECK_FAILS(check_commander_step_tangent_args(h, 1, &in, &cmd, &c), msg(": state_before is required (the commander records from before the forward call)"),
                "no state_before");
    CHECK(check_commander_step_tangent_args(h, 0, &in, &cmd, &c) == QC_OK, "n = 0 needs no records");
  }
  for (int k = 0; k < 2; k++) {
    qc_batch_in c = in;
    (k == 0 ? c.Rwb : c.x) = nullptr;
    CHECK_FAILS(check_commander_step_tangent_args(h, 1, &c, &cmd, &io), msg(": Rwb and x are required"), "missing array %d", k);
  }
  {
    const size_t cap = (size_t)0xFFFFFF * (size_t)COMMAND_TANGENT_BLOCK;
    qc_commander_step_tangent_io c = io;
    CHECK(check_commander_step_tangent_args(h, cap, &in, &cmd, &c) == QC_OK, "n at the launch bound, K = 1");
    CHECK_FAILS(check_commander_step_tangent_args(h, cap + 1, &in, &cmd, &c), msg(": n is beyond one launch"), "n one past the bound");
    c.n_dir = 2;
    CHECK_FAILS(check_commander_step_tangent_args(h, cap, &in, &cmd, &c), msg(": n * n_dir is beyond one launch"), "n at the bound, K = 2");
    CHECK(check_commander_step_tangent_args(h, cap / 2, &in, &cmd, &c) == QC_OK, "n K at the bound");
    c.n_dir = std::numeric_limits<size_t>::max();
    CHECK_FAILS(check_commander_step_tangent_args(h, 2, &in, &cmd, &c), msg(": n * n_dir is beyond one launch"), "a product that would wrap");
  }
}

static void packing() {
  const qc_batch_in in = valid_in();
  const qc_command_in cmd = valid_cmd();
  qc_commander_step_tangent_io io = valid_io();
  io.n_dir = 5; io.Vb_tan = buf + 5; io.Vb_next_tan = buf + 5; io.flags = ibuf; io.w_d_prev_tan = buf + 6;
  const CommanderStepTangentArgs a = commander_step_tangent_constants(&in, &cmd, &io);
  CHECK(a.Rwb == in.Rwb && a.x == in.x && a.twist == cmd.twist && a.fresh == cmd.fresh && (const void*)a.before == (const void*)records, "the arrays read");
  CHECK(a.stand_height == 0.26 && a.stand_tol == 0.005 && a.cmd_dt == 0.001 && a.n_dir == 5, "the scalars and K");
  CHECK(a.twist_tan == io.twist_tan && a.Vb_tan == io.Vb_tan && !a.Rwb_rot_tan && !a.x_tan && !a.Rwb_d_rot_prev_tan && !a.x_d_prev_tan && !a.xdot_d_prev_tan &&
            a.w_d_prev_tan == io.w_d_prev_tan,
        "the tangents");
  CHECK(!a.Rwb_d_rot_tan && a.x_d_tan == io.x_d_tan && !a.xdot_d_tan && !a.w_d_tan && a.Vb_next_tan == io.Vb_next_tan && a.flags == ibuf, "the outputs");
  CHECK(command_tangent_blocks(1, 1) == 1 && command_tangent_blocks(64, 1) == 1 && command_tangent_blocks(65, 1) == 2 && command_tangent_blocks(22, 3) == 2,
        "one wave of pairs per workgroup");
  const size_t at = (size_t)COMMAND_TANGENT_MAX_BLOCKS * COMMAND_TANGENT_BLOCK;
  CHECK(command_tangent_blocks(at, 1) == (unsigned)COMMAND_TANGENT_MAX_BLOCKS && command_tangent_blocks(at + 1, 1) == (unsigned)COMMAND_TANGENT_MAX_BLOCKS &&
            command_tangent_blocks(at / 4, 4) == (unsigned)COMMAND_TANGENT_MAX_BLOCKS && command_tangent_blocks(at - 64, 1) == (unsigned)COMMAND_TANGENT_MAX_BLOCKS - 1,
        "the grid cap");
}

int main() {
  arguments();
  packing();
  std::printf("commander step tangent host logic ok\n");
  return 0;
}
