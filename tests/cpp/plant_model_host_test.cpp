// The device-free host logic of the plant steps with a model (include/qc_plant_model.h; quadruped_control_amd/csrc/qc_host.hpp):
// every refusal of qc_plant_step_model_batch, qc_leg_plant_step_model_batch and qc_plant_step_model_adjoint_batch, the body's
// constants under a model, and the instantiation a model selects.  Host compiler only - links neither HIP nor the library; built with
// the address and undefined-behaviour sanitizers and run by tests/test_plant_model_cpu.py.  Prints the failing case and exits 1 on the
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
static double buf[16];
static int32_t ibuf[4];
static const qc_handle* const h = reinterpret_cast<const qc_handle*>(buf);  // only compared with null

static qc_plant_model wrench_model() {
  qc_plant_model m{};
  m.struct_size = sizeof(qc_plant_model);
  m.wrench_world = buf;
  return m;
}

// what all three calls refuse about the model, through `call(model)`, under the name `who`; `base`: the call the message points to
template <class Call>
static void model_refusals(const std::string& who, const char* base, Call call) {
  qc_plant_model m = wrench_model();
  CHECK(call(&m) == QC_OK, "%s: a wrench alone", who.c_str());
  for (int v = 1; v < 8; v++) {
    qc_plant_model c{};
    c.struct_size = sizeof(qc_plant_model);
    c.mass = (v & 1) ? buf : nullptr;
    c.Ib = (v & 2) ? buf : nullptr;
    c.wrench_world = (v & 4) ? buf : nullptr;
    CHECK(call(&c) == QC_OK && plant_model_variant(&c) == v, "%s: variant %d", who.c_str(), v);
    c.flags = ibuf;
    CHECK(call(&c) == QC_OK && plant_model_variant(&c) == v, "%s: variant %d with flags", who.c_str(), v);
  }
  CHECK_FAILS(call(nullptr), who + ": null argument", "no model");
  for (const size_t sz : {(size_t)0, sizeof(qc_plant_model) - 8, sizeof(qc_plant_model) + 8}) {
    qc_plant_model c = m;
    c.struct_size = sz;
    char text[224];
    std::snprintf(text, sizeof(text), "%s: qc_plant_model.struct_size is %zu, this library's qc_plant_model has %zu B (qc_default_plant_model sets it)",
                  who.c_str(), sz, sizeof(qc_plant_model));
    CHECK_FAILS(call(&c), std::string(text), "model struct_size %zu", sz);
  }
  {
    qc_plant_model c = m;
    c.wrench_world = nullptr;
    CHECK_FAILS(call(&c), who + ": the model gives neither mass, Ib nor wrench_world - call " + base, "an empty model");
    c.flags = ibuf;
    CHECK_FAILS(call(&c), who + ": the model gives neither mass, Ib nor wrench_world - call " + base, "an empty model with flags");
  }
}

// ------------------------------------------------------------------------------------------------ (a) qc_plant_step_model_batch
static void rigid() {
  const std::string who = "qc_plant_step_model_batch";
  qc_plant_io io{};
  io.struct_size = sizeof(qc_plant_io);
  io.Rwb = io.x = io.xdot = io.w = buf;
  io.grf_body = io.foot_world = buf;
  io.dt = 1.0 / 300.0;
  const qc_plant_model m = wrench_model();
  model_refusals(who, "qc_plant_step_batch", [&](const qc_plant_model* c) { return check_plant_model_args(h, 1, &io, c); });
  // everything the base call refuses, under this call's name, and before the model is looked at
  CHECK_FAILS(check_plant_model_args(nullptr, 1, &io, &m), who + ": null argument", "no handle");
  CHECK_FAILS(check_plant_model_args(h, 1, nullptr, &m), who + ": null argument", "no io");
  {
    qc_plant_io c = io;
    c.struct_size = 8;
    CHECK(check_plant_model_args(h, 1, &c, &m) == QC_ERR_INVALID && g_err.rfind(who + ": qc_plant_io.struct_size is 8", 0) == 0, "io struct_size");
    CHECK(check_plant_model_args(h, 1, &c, nullptr) == QC_ERR_INVALID && g_err.rfind(who + ": qc_plant_io.struct_size is 8", 0) == 0, "io struct_size first");
  }
  for (const double dt : {0.0, -1.0, kInf, kNan}) {
    qc_plant_io c = io;
    c.dt = dt;
    CHECK_FAILS(check_plant_model_args(h, 1, &c, &m), who + ": dt must be finite and > 0", "dt %g", dt);
    CHECK_FAILS(check_plant_model_args(h, 0, &c, &m), who + ": dt must be finite and > 0", "dt %g, n = 0", dt);
  }
  {
    double* qc_plant_io::*const st[] = {&qc_plant_io::Rwb, &qc_plant_io::x, &qc_plant_io::xdot, &qc_plant_io::w};
    for (int i = 0; i < 4; i++) {
      qc_plant_io c = io;
      c.*st[i] = nullptr;
      CHECK_FAILS(check_plant_model_args(h, 1, &c, &m), who + ": the state arrays Rwb, x, xdot and w are required", "state array %d missing", i);
      CHECK(check_plant_model_args(h, 0, &c, &m) == QC_OK, "n = 0 reads no array");
    }
    const double* qc_plant_io::*const in[] = {&qc_plant_io::grf_body, &qc_plant_io::foot_world};
    for (int i = 0; i < 2; i++) {
      qc_plant_io c = io;
      c.*in[i] = nullptr;
      CHECK_FAILS(check_plant_model_args(h, 1, &c, &m), who + ": grf_body and foot_world are required", "input array %d missing", i);
    }
  }
  CHECK(check_plant_model_args(h, (size_t)0xFFFFFF * PLANT_BLOCK, &io, &m) == QC_OK, "the largest launch");
  CHECK_FAILS(check_plant_model_args(h, (size_t)0xFFFFFF * PLANT_BLOCK + 1, &io, &m), who + ": n is beyond one launch", "one robot more");
  CHECK_FAILS(check_plant_model_args(h, 0, &io, nullptr), who + ": null argument", "no model, n = 0");
  {
    qc_plant_model empty = m;
    empty.wrench_world = nullptr;  // what a caller's arrays of no robots look like
    CHECK(check_plant_model_args(h, 0, &io, &empty) == QC_OK, "n = 0 reads no array, of the model's either");
    qc_leg_plant_io lio{};
    lio.struct_size = sizeof(qc_leg_plant_io);
    lio.leg_inertia[0] = lio.leg_inertia[1] = lio.leg_inertia[2] = 0.02;
    lio.dt = io.dt;
    CHECK(check_leg_plant_model_args(h, 0, &lio, &empty) == QC_OK, "leg: n = 0 reads no array");
    qc_plant_adjoint_io aio{};
    aio.struct_size = sizeof(qc_plant_adjoint_io);
    aio.x_next_bar = buf;
    aio.x_bar = buf;
    aio.dt = io.dt;
    CHECK(check_plant_model_adjoint_args(h, 0, &aio, &empty, nullptr) == QC_OK, "adjoint: n = 0 reads no array");
    empty.struct_size = 8;
    CHECK(check_plant_model_args(h, 0, &io, &empty) == QC_ERR_INVALID, "n = 0: the model's revision is still checked");
  }
  CHECK(sizeof(qc_plant_model) == 5 * 8 && sizeof(qc_plant_model_bar) == 5 * 8, "both records: one size field and four pointers");
}

// ------------------------------------------------------------------------------------------------ (b) the body's constants under a model
static void constants() {
  const double Ib[9] = {0.011253, 0, 0, 0, 0.036203, 0, 0, 0, 0.042673}, zero[9] = {}, asym[9] = {1, 0, 0, 0, 1, 0.25, 0, 0, 1};
  const std::string who = "qc_plant_step_model_batch";
  qc_plant_io io{};
  io.dt = 0.002;
  {
    const qc_plant_model m = wrench_model();
    PlantArgs a{}, base{};
    CHECK(plant_model_constants(9.0, Ib, &io, &m, a) == QC_OK && plant_constants(9.0, Ib, &io, base) == QC_OK, "a wrench alone: the handle's body");
    CHECK(a.mass == 9.0 && a.g == PLANT_G && a.dt == 0.002, "mass, g, dt");
    for (int k = 0; k < 9; k++) CHECK(a.Ib[k] == Ib[k] && a.Ib_inv[k] == base.Ib_inv[k], "Ib and the handle's inverse, entry %d", k);
    for (const double mass : {0.0, -1.0, kInf, kNan})
      CHECK_FAILS(plant_model_constants(mass, Ib, &io, &m, a), who + ": the handle's mass is not finite and > 0", "the handle's mass %g", mass);
    CHECK_FAILS(plant_model_constants(9.0, zero, &io, &m, a), who + ": the handle's Ib is not positive definite", "the handle's zero inertia");
    CHECK_FAILS(plant_model_constants(9.0, asym, &io, &m, a), who + ": the handle's Ib is not symmetric", "the handle's asymmetric inertia");
  }
  {  // the model supplies the mass: the handle's is not asked
    qc_plant_model m = wrench_model();
    m.mass = buf;
    PlantArgs a{};
    for (const double mass : {9.0, 0.0, -1.0, kNan}) CHECK(plant_model_constants(mass, Ib, &io, &m, a) == QC_OK && a.mass == 1.0, "the handle's mass %g", mass);
    CHECK_FAILS(plant_model_constants(9.0, zero, &io, &m, a), who + ": the handle's Ib is not positive definite", "Ib is still the handle's");
  }
  {  // the model supplies Ib
    qc_plant_model m = wrench_model();
    m.Ib = buf;
    PlantArgs a{};
    for (const double* I : {Ib, zero, asym}) {
      CHECK(plant_model_constants(9.0, I, &io, &m, a) == QC_OK && a.mass == 9.0, "the handle's Ib is not asked");
      for (int k = 0; k < 9; k++) CHECK(a.Ib[k] == (k % 4 == 0 ? 1.0 : 0.0) && a.Ib_inv[k] == a.Ib[k], "the placeholder, entry %d", k);
    }
    CHECK_FAILS(plant_model_constants(0.0, Ib, &io, &m, a), who + ": the handle's mass is not finite and > 0", "the mass is still the handle's");
    m.mass = buf;
    CHECK(plant_model_constants(kNan, zero, &io, &m, a) == QC_OK, "both from the model: nothing is asked of the handle");
  }
  {  // under the other two names
    const qc_plant_model m = wrench_model();
    qc_leg_plant_io lio{};
    lio.dt = 0.002;
    lio.leg_inertia[0] = 0.02; lio.leg_inertia[1] = 0.03; lio.leg_inertia[2] = 0.025;
    lio.foot_world = buf;
    lio.flags = ibuf;
    LegPlantArgs l{}, lbase{};
    CHECK(leg_plant_model_constants(9.0, Ib, &lio, &m, l) == QC_OK && leg_plant_constants(9.0, Ib, &lio, lbase) == QC_OK, "the leg plant's arguments");
    CHECK(std::memcmp(&l, &lbase, sizeof(l)) == 0, "a wrench alone: the base call's argument struct, byte for byte");
    CHECK_FAILS(leg_plant_model_constants(0.0, Ib, &lio, &m, l), "qc_leg_plant_step_model_batch: the handle's mass is not finite and > 0", "leg: mass 0");
    qc_plant_adjoint_io aio{};
    aio.dt = 0.002;
    aio.Rwb = aio.x = buf;
    aio.x_next_bar = buf;
    aio.grf_bar = buf;
    PlantAdjointArgs ad{}, abase{};
    CHECK(plant_model_adjoint_constants(9.0, Ib, &aio, &m, ad) == QC_OK && plant_adjoint_constants(9.0, Ib, &aio, abase) == QC_OK, "the adjoint's arguments");
    CHECK(std::memcmp(&ad, &abase, sizeof(ad)) == 0, "a wrench alone: the base adjoint's argument struct, byte for byte");
    CHECK_FAILS(plant_model_adjoint_constants(9.0, zero, &aio, &m, ad), "qc_plant_step_model_adjoint_batch: the handle's Ib is not positive definite", "adjoint: zero Ib");
  }
  {
    qc_plant_model m = wrench_model();
    m.mass = buf + 1; m.Ib = buf + 2; m.flags = ibuf;
    const PlantModelArgs a = plant_model_args(&m);
    CHECK(a.mass == buf + 1 && a.Ib == buf + 2 && a.wrench == buf && a.flags == ibuf, "the model's pointers travel as given");
    qc_plant_model_bar b{};
    b.wrench_bar = buf; b.mass_bar = buf + 1; b.Ib_bar = buf + 2; b.flags = ibuf;
    const PlantModelBarArgs ba = plant_model_bar_args(&b), none = plant_model_bar_args(nullptr);
    CHECK(ba.wrench_bar == buf && ba.mass_bar == buf + 1 && ba.Ib_bar == buf + 2 && ba.flags == ibuf, "the bar's pointers travel as given");
    CHECK(!none.wrench_bar && !none.mass_bar && !none.Ib_bar && !none.flags, "no bar: no output");
  }
}

// ------------------------------------------------------------------------------------------------ (c) qc_leg_plant_step_model_batch
static void legged() {
  const std::string who = "qc_leg_plant_step_model_batch";
  qc_leg_plant_io io{};
  io.struct_size = sizeof(qc_leg_plant_io);
  io.Rwb = io.x = io.xdot = io.w = io.joint_q = io.joint_qdot = buf;
  io.joint_tau = buf;
  io.leg_inertia[0] = 0.02; io.leg_inertia[1] = 0.03; io.leg_inertia[2] = 0.025;
  io.dt = 1.0 / 300.0;
  const qc_plant_model m = wrench_model();
  model_refusals(who, "qc_leg_plant_step_batch", [&](const qc_plant_model* c) { return check_leg_plant_model_args(h, 1, &io, c); });
  CHECK_FAILS(check_leg_plant_model_args(nullptr, 1, &io, &m), who + ": null argument", "no handle");
  CHECK_FAILS(check_leg_plant_model_args(h, 1, nullptr, &m), who + ": null argument", "no io");
  {
    qc_leg_plant_io c = io;
    c.struct_size = 8;
    CHECK(check_leg_plant_model_args(h, 1, &c, &m) == QC_ERR_INVALID && g_err.rfind(who + ": qc_leg_plant_io.struct_size is 8", 0) == 0, "io struct_size");
  }
  for (const double dt : {0.0, -1.0, kInf, kNan}) {
    qc_leg_plant_io c = io;
    c.dt = dt;
    CHECK_FAILS(check_leg_plant_model_args(h, 1, &c, &m), who + ": dt must be finite and > 0", "dt %g", dt);
  }
  for (int k = 0; k < 3; k++)
    for (const double bad : {0.0, -0.02, kInf, kNan}) {
      qc_leg_plant_io c = io;
      c.leg_inertia[k] = bad;
      CHECK_FAILS(check_leg_plant_model_args(h, 1, &c, &m),
                  who + ": leg_inertia (hip, thigh, calf) must be finite and > 0; qc_default_leg_plant leaves it at 0, the caller gives it", "leg_inertia[%d] = %g", k, bad);
    }
  {
    double* qc_leg_plant_io::*const st[] = {&qc_leg_plant_io::Rwb, &qc_leg_plant_io::x, &qc_leg_plant_io::xdot, &qc_leg_plant_io::w};
    for (int i = 0; i < 4; i++) {
      qc_leg_plant_io c = io;
      c.*st[i] = nullptr;
      CHECK_FAILS(check_leg_plant_model_args(h, 1, &c, &m), who + ": the state arrays Rwb, x, xdot and w are required", "state array %d missing", i);
    }
    for (int i = 0; i < 3; i++) {
      qc_leg_plant_io c = io;
      if (i == 0) c.joint_q = nullptr;
      if (i == 1) c.joint_qdot = nullptr;
      if (i == 2) c.joint_tau = nullptr;
      CHECK_FAILS(check_leg_plant_model_args(h, 1, &c, &m), who + ": joint_q, joint_qdot and joint_tau are required", "joint array %d missing", i);
      CHECK(check_leg_plant_model_args(h, 0, &c, &m) == QC_OK, "n = 0 reads no array");
    }
  }
  CHECK_FAILS(check_leg_plant_model_args(h, (size_t)0xFFFFFF * LEG_PLANT_BLOCK + 1, &io, &m), who + ": n is beyond one launch", "one robot more");
}

// ------------------------------------------------------------------------------------------------ (d) qc_plant_step_model_adjoint_batch
static void adjoint() {
  const std::string who = "qc_plant_step_model_adjoint_batch";
  qc_plant_adjoint_io io{};
  io.struct_size = sizeof(qc_plant_adjoint_io);
  io.Rwb = io.x = io.xdot = io.w = io.grf_body = io.foot_world = buf;
  io.x_next_bar = buf;
  io.x_bar = buf;
  io.dt = 1.0 / 300.0;
  const qc_plant_model m = wrench_model();
  qc_plant_model_bar bar{};
  bar.struct_size = sizeof(qc_plant_model_bar);
  model_refusals(who, "qc_plant_step_adjoint_batch", [&](const qc_plant_model* c) { return check_plant_model_adjoint_args(h, 1, &io, c, nullptr); });
  model_refusals(who, "qc_plant_step_adjoint_batch", [&](const qc_plant_model* c) { return check_plant_model_adjoint_args(h, 1, &io, c, &bar); });
  CHECK_FAILS(check_plant_model_adjoint_args(nullptr, 1, &io, &m, &bar), who + ": null argument", "no handle");
  CHECK_FAILS(check_plant_model_adjoint_args(h, 1, nullptr, &m, &bar), who + ": null argument", "no io");
  {
    qc_plant_adjoint_io c = io;
    c.struct_size = 8;
    CHECK(check_plant_model_adjoint_args(h, 1, &c, &m, &bar) == QC_ERR_INVALID && g_err.rfind(who + ": qc_plant_adjoint_io.struct_size is 8", 0) == 0, "io struct_size");
  }
  for (const size_t sz : {(size_t)0, sizeof(qc_plant_model_bar) - 8, sizeof(qc_plant_model_bar) + 8}) {
    qc_plant_model_bar c = bar;
    c.struct_size = sz;
    char text[224];
    std::snprintf(text, sizeof(text), "%s: qc_plant_model_bar.struct_size is %zu, this library's qc_plant_model_bar has %zu B (qc_default_plant_model_bar sets it)",
                  who.c_str(), sz, sizeof(qc_plant_model_bar));
    CHECK_FAILS(check_plant_model_adjoint_args(h, 1, &io, &m, &c), std::string(text), "bar struct_size %zu", sz);
  }
  for (const double dt : {0.0, -1.0, kInf, kNan}) {
    qc_plant_adjoint_io c = io;
    c.dt = dt;
    CHECK_FAILS(check_plant_model_adjoint_args(h, 1, &c, &m, &bar), who + ": dt must be finite and > 0", "dt %g", dt);
  }
  {
    qc_plant_adjoint_io c = io;
    c.x_next_bar = nullptr;
    CHECK_FAILS(check_plant_model_adjoint_args(h, 1, &c, &m, &bar),
                who + ": no input cotangent given (Rwb_next_bar, x_next_bar, xdot_next_bar, w_next_bar, feet_next_bar are all NULL)", "no cotangent");
  }
  {  // an output of either record will do
    const std::string none = who + ": no output requested (Rwb_bar, x_bar, xdot_bar, w_bar, grf_bar, foot_world_bar and the model's wrench_bar, mass_bar, Ib_bar are all NULL)";
    qc_plant_adjoint_io c = io;
    c.x_bar = nullptr;
    CHECK_FAILS(check_plant_model_adjoint_args(h, 1, &c, &m, nullptr), none, "no output, no bar");
    CHECK_FAILS(check_plant_model_adjoint_args(h, 1, &c, &m, &bar), none, "no output, an empty bar");
    qc_plant_model_bar f = bar;
    f.flags = ibuf;
    CHECK_FAILS(check_plant_model_adjoint_args(h, 1, &c, &m, &f), none, "flags alone are no output");
    for (int k = 0; k < 3; k++) {
      qc_plant_model_bar b = bar;
      if (k == 0) b.wrench_bar = buf;
      if (k == 1) b.mass_bar = buf;
      if (k == 2) b.Ib_bar = buf;
      CHECK(check_plant_model_adjoint_args(h, 1, &c, &m, &b) == QC_OK, "the bar's output %d alone", k);
    }
    CHECK(check_plant_model_adjoint_args(h, 1, &io, &m, nullptr) == QC_OK, "the record's output alone, bar NULL");
  }
  {
    const double* qc_plant_adjoint_io::*const in[] = {&qc_plant_adjoint_io::Rwb, &qc_plant_adjoint_io::x, &qc_plant_adjoint_io::xdot, &qc_plant_adjoint_io::w};
    for (int i = 0; i < 4; i++) {
      qc_plant_adjoint_io c = io;
      c.*in[i] = nullptr;
      CHECK_FAILS(check_plant_model_adjoint_args(h, 1, &c, &m, &bar), who + ": the state arrays Rwb, x, xdot and w are required", "state array %d missing", i);
      CHECK(check_plant_model_adjoint_args(h, 0, &c, &m, &bar) == QC_OK, "n = 0 reads no array");
    }
    const double* qc_plant_adjoint_io::*const other[] = {&qc_plant_adjoint_io::grf_body, &qc_plant_adjoint_io::foot_world};
    for (int i = 0; i < 2; i++) {
      qc_plant_adjoint_io c = io;
      c.*other[i] = nullptr;
      CHECK_FAILS(check_plant_model_adjoint_args(h, 1, &c, &m, &bar), who + ": grf_body and foot_world are required", "input array %d missing", i);
    }
  }
  CHECK_FAILS(check_plant_model_adjoint_args(h, (size_t)0xFFFFFF * PLANT_BLOCK + 1, &io, &m, &bar), who + ": n is beyond one launch", "one robot more");
}

int main() {
  rigid();
  constants();
  legged();
  adjoint();
  std::printf("plant model host logic ok: %ld checks\n", g_checked);
  return 0;
}
