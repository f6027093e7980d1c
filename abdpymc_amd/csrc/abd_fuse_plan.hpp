// abd_fuse_plan.hpp -- how abd_logp_dlogp_many cuts the K steps of a call into launches (abd_eval.hip).  Plain C++, no HIP:
// tests/native/fuse_plan_harness.cpp runs it on the CPU.
//
// A dense launch carries S consecutive steps of n chains as S times as many grid rows of 1 / S as many ranges each (the
// kernel's per-range work -- set-up, tables, start state, reduction -- is then paid once per S steps' share of the plane).
// S depends on (K, n, pipes) only, never on timing, so a call's numbers are repeatable.
#pragma once

#include <algorithm>
#include <vector>

namespace abdi {

constexpr int kFuseMaxSteps = 4;  // steps of one launch at most
// a call fuses S steps only if every pipe still gets this many launches, so the driver's K = 20 protocol keeps the launches it
// always had.  Measured (profiles/README.md, r05, f_fuse_sweep_*.txt): S = 4 is the fastest at K = 500, 100 and 20; why short
// calls are left alone all the same is in DESIGN.md section 9
constexpr int kFuseMinLaunchesPerPipe = 4;

struct FusedLaunch {
  int first;   // first step of the launch
  int steps;   // consecutive steps it carries
  bool alone;  // the last launch of the call: it ends alone on the chip and gets the grid of a launch that has it to itself
};

// steps per launch of a call of K steps of n chains over `pipes` pipes; forced: 0 = the rule, else that many (capped by
// the rows of a launch); max_steps: what the caller's buffers allow (1 = never fuse)
inline int fuse_steps(int K, int n, int pipes, int forced, int max_steps = kFuseMaxSteps, int max_rows = 16) {
  if (n < 1 || n > max_rows) return 1;  // a step of more than max_rows chains already needs several launches
  const int room = std::max(1, std::min({kFuseMaxSteps, max_steps, max_rows / n}));
  if (forced > 0) return std::min(forced, room);
  for (int s = room; s > 1; --s)
    if ((long long)K >= (long long)kFuseMinLaunchesPerPipe * s * std::max(1, pipes)) return s;
  return 1;
}

// the launches of the call in order; none crosses a window of `ring` result slots
inline std::vector<FusedLaunch> fuse_plan(int K, int n, int pipes, int ring, int forced, int max_steps = kFuseMaxSteps, int max_rows = 16) {
  std::vector<FusedLaunch> plan;
  if (K <= 0) return plan;
  const int S = fuse_steps(K, n, pipes, forced, max_steps, max_rows);
  ring = std::max(1, ring);
  plan.reserve((size_t)(K / S + K / ring + 2));
  for (long long w0 = 0; w0 < K; w0 += ring) {
    const long long w1 = std::min<long long>(K, w0 + ring);
    for (long long k = w0; k < w1; k += S) plan.push_back({(int)k, (int)std::min<long long>(S, w1 - k), false});
  }
  plan.back().alone = true;
  return plan;
}

}  // namespace abdi
