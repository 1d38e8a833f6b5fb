// What the stand-alone host-logic programs of this directory share: a counter of the checks made and the two check macros.  A
// violated check prints the failing case with the library's last error and exits 1.
#pragma once
#include <cstdio>
#include <cstdlib>

#include "../../quadruped_control_amd/csrc/qc_host.hpp"

static long g_checked = 0;
#define CHECK(cond, ...)                                              \
  do {                                                                \
    g_checked++;                                                      \
    if (!(cond)) {                                                    \
      std::printf("FAILED %s:%d: %s\n  case: ", __FILE__, __LINE__, #cond); \
      std::printf(__VA_ARGS__);                                       \
      std::printf("\n  last error: %s\n", qc::g_err.c_str());         \
      std::exit(1);                                                   \
    }                                                                 \
  } while (0)
// a call that must fail with QC_ERR_INVALID and exactly this text
#define CHECK_FAILS(rc, text, ...) CHECK((rc) == QC_ERR_INVALID && qc::g_err == (text), __VA_ARGS__)
