// The device-resident scalar chain behind kry_prog (blas.hip), shared with the
// translation units that enqueue chain steps of their own (tri.hip).
#pragma once

#include "solver_common.hpp"

struct kry_prog {
  kry_ctx *ctx = nullptr;
  int nregs = 0, k = 1, cap = 0;
  double *regs = nullptr;  // nregs x k
  double *crit = nullptr;  // k
  double *hist = nullptr;  // cap x k
  double *part = nullptr;  // part_rows(k) x k (the dots' first stage)
  kry::Ctrl *ctrl = nullptr;
};
