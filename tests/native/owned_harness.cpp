// Ownership of the four handles of abd_owned.hpp, on the CPU against tests/native/fake_hip (malloc-backed HIP calls that count
// what is alive and can be told to fail), under AddressSanitizer and UBSan: a double release or a lost block ends the run.
#include <cstdio>
#include <utility>
#include <vector>

#include "abd_owned.hpp"

using namespace abdi;

static int failures = 0;
#define CHECK(cond)                                                          \
  do {                                                                       \
    if (!(cond)) {                                                           \
      std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
      ++failures;                                                            \
    }                                                                        \
  } while (0)

static long live() { return fake_hip::live; }

// what every handle has in common: `make(h)` fills an empty handle with one resource
template <typename H, typename Make>
static void check_handle(Make make) {
  const long base = live();
  {
    H empty;  // destroying an empty handle is a no-op
    CHECK(!empty);
  }
  CHECK(live() == base);
  {
    H a;
    CHECK(make(a) == hipSuccess);
    CHECK(a && live() == base + 1);
    const auto raw = static_cast<decltype(+a)>(a);  // (unary plus: the raw pointer / HIP handle it converts to)
    H b(std::move(a));                              // move construction: one owner, the source empty
    CHECK(!a && static_cast<decltype(+b)>(b) == raw && live() == base + 1);
    H c;
    CHECK(make(c) == hipSuccess && live() == base + 2);
    c = std::move(b);  // move assignment: the target's old resource goes, the source is empty
    CHECK(!b && static_cast<decltype(+c)>(c) == raw && live() == base + 1);
    c = std::move(c);  // onto itself: kept
    CHECK(static_cast<decltype(+c)>(c) == raw && live() == base + 1);
    CHECK(make(c) == hipSuccess && live() == base + 1);  // creating again releases what it held
    H d, e;
    CHECK(make(d) == hipSuccess && live() == base + 2);
    const auto raw_c = static_cast<decltype(+c)>(c), raw_d = static_cast<decltype(+d)>(d);
    std::swap(c, d);
    CHECK(static_cast<decltype(+c)>(c) == raw_d && static_cast<decltype(+d)>(d) == raw_c && live() == base + 2);
    std::swap(d, e);  // with an empty one
    CHECK(!d && static_cast<decltype(+e)>(e) == raw_c && live() == base + 2);
    c.reset();
    CHECK(!c && live() == base + 1);
    fake_hip::fail_at = fake_hip::calls + 1;  // a failing create leaves the handle empty, whatever it held
    CHECK(make(e) != hipSuccess && !e && live() == base);
  }
  CHECK(live() == base);  // scope exit
}

// a chain slot and a pipe as the context keeps them
struct Slot {
  DevBuf<unsigned long long> rw;
  DevBuf<signed char> waner;
  MappedBuf<double> rec;
  bool set = false;
};
struct Pipe {
  Stream st;
  DevBuf<double> partials[2];
  Event join;
};
struct Owner {
  Pipe pipe[3];
  std::vector<Slot> slots;
  std::vector<std::pair<Event, Event>> ev_pool;
};
static constexpr int kBuildCalls = 3 * 4 + 4 * 3 + 2;  // the create / allocate calls of one build()

// built the way abd_create builds a context: any step may fail, and the caller just returns
static hipError_t build(Owner& o) {
  for (Pipe& p : o.pipe) {
    if (hipError_t e = p.st.create()) return e;
    if (hipError_t e = p.join.create()) return e;
    for (auto& b : p.partials)
      if (hipError_t e = b.alloc(16)) return e;
  }
  o.slots.resize(4);
  for (Slot& s : o.slots) {
    if (hipError_t e = s.rw.alloc(8)) return e;
    if (hipError_t e = s.waner.alloc_zero(5, o.pipe[0].st)) return e;
    if (hipError_t e = s.rec.alloc(3)) return e;
  }
  Event a0, a1;
  if (hipError_t e = a0.create()) return e;
  if (hipError_t e = a1.create()) return e;  // (the first event is not lost when the second fails)
  o.ev_pool.emplace_back(std::move(a0), std::move(a1));
  return hipSuccess;
}

int main() {
  check_handle<DevBuf<double>>([](DevBuf<double>& b) { return b.alloc(7); });
  check_handle<DevBuf<unsigned char>>([](DevBuf<unsigned char>& b) { return b.alloc_zero(3, nullptr); });
  check_handle<MappedBuf<double>>([](MappedBuf<double>& b) { return b.alloc(5); });
  check_handle<MappedBuf<long>>([](MappedBuf<long>& b) { return b.alloc_pinned(5); });
  check_handle<Stream>([](Stream& s) { return s.create(); });
  check_handle<Event>([](Event& e) { return e.create(); });

  {  // contents: zeroed, uploaded, both views of mapped memory, host view only of plain pinned memory
    DevBuf<int> z;
    CHECK(z.alloc_zero(4, nullptr) == hipSuccess && z[0] == 0 && z[3] == 0);
    const int src[3] = {4, 5, 6};
    CHECK(z.upload(src, 3) == hipSuccess && z[0] == 4 && z[2] == 6 && live() == 1);
    MappedBuf<double> m, p;
    CHECK(m.alloc(4) == hipSuccess && m.host() && m.dev() == m.host() && m.host()[3] == 0.0);
    CHECK(p.alloc_pinned(4) == hipSuccess && p.host() && !p.dev() && p.host()[3] == 0.0);
    MappedBuf<double> q(std::move(m));
    CHECK(!m.host() && !m.dev() && q.host() && q.dev());
    p = std::move(q);
    CHECK(!q.host() && !q.dev() && p.dev() && live() == 2);
  }
  CHECK(live() == 0);

  {  // a vector of slots that grows (its elements move), shrinks and goes
    std::vector<Slot> v(2);
    for (Slot& s : v) CHECK(s.rw.alloc(4) == hipSuccess && s.rec.alloc(2) == hipSuccess);
    CHECK(live() == 4);
    const unsigned long long* first = v[0].rw;
    v.resize(50);
    CHECK(live() == 4 && v[0].rw == first && !v[49].rw);
    for (Slot& s : v) CHECK(s.waner.alloc(1) == hipSuccess);
    CHECK(live() == 54);
    v.resize(1);
    CHECK(live() == 3);
  }
  CHECK(live() == 0);

  {  // the whole build, then every early return of it: whichever call fails, nothing outlives the owner
    Owner whole;
    const long c0 = fake_hip::calls;
    CHECK(build(whole) == hipSuccess && fake_hip::calls - c0 == kBuildCalls && live() == kBuildCalls);
  }
  CHECK(live() == 0);
  for (int k = 1; k <= kBuildCalls; ++k) {
    {
      Owner o;
      fake_hip::fail_at = fake_hip::calls + k;
      CHECK(build(o) == hipErrorOutOfMemory);
      // everything made before the failing call is still owned -- by o, except the first event of the pair, which went
      // with build()'s local handle when the second failed
      CHECK(live() == (k < kBuildCalls ? k - 1 : k - 2));
    }
    CHECK(live() == 0);
  }
  if (failures) return 1;
  std::puts("owned ok");
  return 0;
}
