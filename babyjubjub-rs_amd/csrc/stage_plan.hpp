// stage_plan.hpp -- where the arrays of ONE staged call lie in a block of a scratch set (bjj_hip.hip: Staged, the synchronous
// single-launch host forms): an optional scratch prefix (a kernel layout's bytes), then the arrays in the order they are declared,
// the inputs before the outputs, each at the next multiple of 256; an absent array (count 0) takes no space.  An array may also be
// declared at a given offset INSIDE the prefix (the MSM forms read their results out of the kernel's own layout).  Pure functions of
// plain values: no HIP, no heap.  Also built for the CPU under AddressSanitizer / UBSan by tests/test_stage_plan.py
// (tests/emul/emul_stage_plan.cpp).
#pragma once
#include <stddef.h>
#include "pipe_plan.hpp"   // up256

#define STAGE_MAX_ARRAYS 9   // bjj_mul_bases: BJJ_MAX_BASES scalar arrays and the results (asserted in bjj_hip.hip)

struct StagePlan {
  struct Array { size_t off, bytes; bool out; };
  Array a[STAGE_MAX_ARRAYS] = {};
  int n = 0;
  size_t end;                                   // the end of the last array behind the prefix (the prefix's while there is none)
  explicit StagePlan(size_t prefix = 0) : end(prefix) {}
  // count items of width bytes behind what is there; -> the array's index, -1 when the plan is full
  int add(bool out, size_t count, size_t width) {
    const size_t off = up256(end);
    const int i = at(out, off, count * width);
    if (i >= 0 && count * width) end = off + count * width;
    return i;
  }
  // ... at a given offset, inside the prefix: takes no space
  int at(bool out, size_t off, size_t bytes) {
    if (n == STAGE_MAX_ARRAYS) return -1;
    a[n] = {off, bytes, out};
    return n++;
  }
  // what the call allocates: the end of the last array as it is, or rounded up like the arrays before it
  size_t total(bool round_last) const { return round_last ? up256(end) : end; }
};
