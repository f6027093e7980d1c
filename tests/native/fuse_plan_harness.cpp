// The launch plan of abd_logp_dlogp_many (abd_fuse_plan.hpp) on the CPU, under AddressSanitizer and UBSan
// (tests/test_fuse_plan_native.py).
#include <cstdio>
#include <vector>

#include "abd_fuse_plan.hpp"

using namespace abdi;

static int fails = 0;
#define CHECK(cond, ...)                                   \
  do {                                                     \
    if (!(cond)) {                                         \
      std::printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); \
      std::printf(__VA_ARGS__);                            \
      std::printf("\n");                                   \
      ++fails;                                             \
    }                                                      \
  } while (0)

static void check_plan(int K, int n, int pipes, int ring, int forced, int max_steps) {
  const std::vector<FusedLaunch> plan = fuse_plan(K, n, pipes, ring, forced, max_steps);
  const int S = fuse_steps(K, n, pipes, forced, max_steps);
  int next = 0;
  for (size_t q = 0; q < plan.size(); ++q) {
    const FusedLaunch& l = plan[q];
    // every step exactly once and in order
    CHECK(l.first == next, "K=%d n=%d pipes=%d forced=%d: launch %zu starts at %d, not %d", K, n, pipes, forced, q, l.first, next);
    CHECK(l.steps >= 1 && l.steps <= S && l.steps <= kFuseMaxSteps, "K=%d n=%d: launch %zu has %d steps (S=%d)", K, n, q, l.steps, S);
    CHECK(n > 16 || n * l.steps <= 16, "K=%d n=%d: launch %zu has %d rows", K, n, q, n * l.steps);
    CHECK(l.steps <= max_steps, "K=%d n=%d: launch %zu has %d steps, the buffers allow %d", K, n, q, l.steps, max_steps);
    // no launch crosses a ring window
    CHECK(l.first / ring == (l.first + l.steps - 1) / ring, "K=%d n=%d: launch %zu [%d, %d) crosses a window of %d", K, n, q, l.first,
          l.first + l.steps, ring);
    // only the last launch of the call has the alone shape
    CHECK(l.alone == (q + 1 == plan.size()), "K=%d n=%d: launch %zu of %zu alone=%d", K, n, q, plan.size(), (int)l.alone);
    if (n > 16) CHECK(l.steps == 1, "K=%d n=%d: a step of more than 16 chains fused", K, n);
    if (forced == 1 || max_steps == 1) CHECK(l.steps == 1, "K=%d n=%d forced=%d max_steps=%d: %d steps", K, n, forced, max_steps, l.steps);
    // a launch is short only where a window or the call ends
    if (l.steps < S) CHECK((l.first + l.steps) % ring == 0 || l.first + l.steps == K, "K=%d n=%d: short launch %zu inside a window", K, n, q);
    next = l.first + l.steps;
  }
  CHECK(next == (K > 0 ? K : 0), "K=%d n=%d: the plan covers %d steps", K, n, next);
  if (forced == 1) CHECK((int)plan.size() == (K > 0 ? K : 0), "K=%d n=%d forced 1: %zu launches", K, n, plan.size());
}

int main() {
  const int Ks[] = {0, 1, 3, 4, 5, 19, 20, 21, 500, 1023, 1024, 1025, 1061};
  const int ns[] = {1, 2, 3, 4, 5, 8, 16, 17};
  for (int K : Ks)
    for (int n : ns)
      for (int pipes : {1, 2, 4, 8})
        for (int ring : {1024, 7})
          for (int forced : {0, 1, 2, 4})
            for (int max_steps : {4, 2, 1}) check_plan(K, n, pipes, ring, forced, max_steps);

  // the rule: S from (K, n, pipes) alone; every pipe keeps kFuseMinLaunchesPerPipe launches
  CHECK(fuse_steps(500, 4, 4, 0) == 4, "config 3 at K = 500");
  CHECK(fuse_steps(100, 4, 4, 0) == 4, "config 3 at K = 100");
  CHECK(fuse_steps(20, 4, 4, 0) == 1, "the K = 20 protocol keeps single steps");
  const int m = kFuseMinLaunchesPerPipe;
  CHECK(fuse_steps(m * 4 * 4 - 1, 4, 4, 0) == 3, "below the threshold of S = 4");
  CHECK(fuse_steps(m * 4 * 4, 4, 4, 0) == 4, "at the threshold of S = 4");
  CHECK(fuse_steps(m * 2 * 4 - 1, 4, 4, 0) == 1 && fuse_steps(m * 2 * 4, 4, 4, 0) == 2, "the threshold of S = 2");
  CHECK(fuse_steps(m * 4 - 1, 4, 1, 0) == 3 && fuse_steps(m * 4, 4, 1, 0) == 4 && fuse_steps(1, 4, 1, 0) == 1, "one pipe");
  CHECK(fuse_steps(500, 5, 4, 0) == 3, "5 chains: 3 steps are 15 rows");
  CHECK(fuse_steps(500, 8, 4, 0) == 2, "8 chains");
  CHECK(fuse_steps(500, 16, 4, 0) == 1, "16 chains fill a launch");
  CHECK(fuse_steps(500, 17, 4, 0) == 1 && fuse_steps(500, 17, 4, 4) == 1, "17 chains never fuse");
  CHECK(fuse_steps(3, 4, 4, 4) == 4 && fuse_steps(3, 4, 4, 2) == 2, "forced values hold whatever K");
  CHECK(fuse_steps(500, 8, 4, 4) == 2, "a forced value is capped by the rows of a launch");
  CHECK(fuse_steps(500, 4, 4, 0, 1) == 1 && fuse_steps(500, 4, 4, 4, 2) == 2, "max_steps caps the rule and the forced value");
  CHECK(fuse_steps(500, 0, 4, 0) == 1, "n = 0");
  CHECK(fuse_plan(-3, 4, 4, 1024, 0).empty() && fuse_plan(0, 4, 4, 1024, 0).empty(), "no steps, no launches");
  {  // a window ends inside what would be a group: 1024 = 341 x 3 + 1
    const std::vector<FusedLaunch> p = fuse_plan(1061, 5, 4, 1024, 0);
    CHECK(p.size() == 342 + 13 && p[341].first == 1023 && p[341].steps == 1 && p[342].first == 1024 && p[342].steps == 3 && p.back().steps == 1,
          "windows of 1024 slots, groups of 3: %zu launches", p.size());
  }
  if (fails) {
    std::printf("%d checks failed\n", fails);
    return 1;
  }
  std::printf("fuse plan ok\n");
  return 0;
}
