// Test infrastructure (CPU box only): what the stand-alone sanitizer drivers of the calls that take no handle share
// (driver_predictive.cpp, driver_top.cpp, driver_foldin.cpp): the hooks of hip_stub.cpp and the two checks of a call's status.
// Such a call owns everything it makes, so a refusal must leave no allocation behind.
#pragma once
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "bnmtf_hip.h"

extern "C" long hipstub_launches();
extern "C" long hipstub_live_allocs();
extern "C" void hipstub_throw_at_sync(long n);

#define OK(expr)                                                                                     \
  do {                                                                                               \
    const int rc_ = (expr);                                                                          \
    if (rc_ != BNMTF_OK) { fprintf(stderr, "FAILED %s -> %d (%s)\n", #expr, rc_, bnmtf_last_error()); exit(2); } \
  } while (0)
#define EXPECT_ERR(expr, text)                                                                       \
  do {                                                                                               \
    const int rc_ = (expr);                                                                          \
    if (rc_ == BNMTF_OK) { fprintf(stderr, "expected an error: %s\n", #expr); exit(2); }             \
    if (!strstr(bnmtf_last_error(), text)) { fprintf(stderr, "%s: the message \"%s\" lacks \"%s\"\n", #expr, bnmtf_last_error(), text); exit(2); } \
    if (hipstub_live_allocs() != 0) { fprintf(stderr, "%s left %ld allocations\n", #expr, hipstub_live_allocs()); exit(2); } \
  } while (0)
