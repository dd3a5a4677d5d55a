// CPU check of the buffer owner in wiser_amd/csrc/dev_mem.h (tests/test_dev_mem.py):
// the growth class over a malloc-backed policy that keeps the set of live
// blocks, aborts on a free of a block it does not hold, and can be told to
// fail the n-th allocation.  One "ok <case>" line per case; exit status 0.
#define WSR_DEV_MEM_NO_HIP
#include "../../wiser_amd/csrc/dev_mem.h"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <new>
#include <set>
#include <utility>

namespace {

struct Fake {
  static std::set<void*> live;
  static int allocs, frees;
  static int fail_at;   // fail the allocation that makes `allocs` this (0: none)
  static void* allocate(size_t bytes) {
    if (++allocs == fail_at) throw std::bad_alloc();
    void* p = std::malloc(bytes ? bytes : 1);
    if (!p) throw std::bad_alloc();
    live.insert(p);
    return p;
  }
  static void release(void* p) {
    if (!live.erase(p)) {
      std::fprintf(stderr, "dev_mem_check: free of a block that is not live: %p\n", p);
      std::abort();
    }
    ++frees;
    std::free(p);
  }
  static void fail_next(int n) { fail_at = allocs + n; }
};
std::set<void*> Fake::live;
int Fake::allocs = 0, Fake::frees = 0, Fake::fail_at = 0;

using Buf = gpu::DevBuf<uint32_t, Fake>;
using Buf64 = gpu::DevBuf<uint64_t, Fake>;

#define CHECK(cond)                                                                  \
  do {                                                                               \
    if (!(cond)) {                                                                   \
      std::fprintf(stderr, "dev_mem_check: %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                                  \
    }                                                                                \
  } while (0)

void ok(const char* name) {
  CHECK(Fake::live.empty());   // every case's buffers are gone by now
  std::printf("ok %s\n", name);
}

void reserve_case() {
  {
    Buf b;
    CHECK(b.get() == nullptr && b.size() == 0 && b.bytes() == 0);
    CHECK(!b.reserve(0, 64) && b.get() == nullptr);   // nothing needed: nothing allocated
    CHECK(b.reserve(10, 16) && b.size() == 16 && b.bytes() == 64 && b.get() != nullptr);
    CHECK(Fake::live.size() == 1);
    uint32_t* p = b.get();
    const int a = Fake::allocs, f = Fake::frees;
    CHECK(!b.reserve(5, 1000) && b.get() == p && b.size() == 16);    // below
    CHECK(!b.reserve(16, 1000) && b.get() == p && b.size() == 16);   // at
    CHECK(Fake::allocs == a && Fake::frees == f);
    CHECK(b.reserve(17, 17 + 17 / 4 + 4096) && b.size() == 17 + 17 / 4 + 4096);   // above: exactly cap_for_need
    CHECK(Fake::allocs == a + 1 && Fake::frees == f + 1 && Fake::live.size() == 1);
    b.alloc(3);   // (alloc sizes exactly, also downwards)
    CHECK(b.size() == 3 && Fake::live.size() == 1);
    b.reset();
    CHECK(b.get() == nullptr && b.size() == 0 && Fake::live.empty());
    b.reset();   // (an empty one: nothing to free)
  }
  ok("reserve");
}

void failed_alloc_case() {
  {
    Buf b;
    b.alloc(100);
    const int f = Fake::frees;
    Fake::fail_next(1);
    bool threw = false;
    try {
      b.reserve(200, 250);
    } catch (const std::bad_alloc&) {
      threw = true;
    }
    CHECK(threw);
    CHECK(b.get() == nullptr && b.size() == 0);           // empty: not dangling, no capacity it does not hold
    CHECK(Fake::frees == f + 1 && Fake::live.empty());    // the old block freed exactly once
    CHECK(b.reserve(50, 60) && b.size() == 60 && b.get() != nullptr);   // a smaller need allocates again
    CHECK(Fake::live.size() == 1);
  }
  ok("failed_alloc");
}

void group_case() {
  {
    Buf a, b;
    Buf64 c;
    gpu::alloc_group(8, a, b, c);
    CHECK(a.size() == 8 && b.size() == 8 && c.size() == 8 && c.bytes() == 64 && Fake::live.size() == 3);
    Fake::fail_next(2);   // the second allocation of the regrowth
    bool threw = false;
    try {
      gpu::alloc_group(32, a, b, c);
    } catch (const std::bad_alloc&) {
      threw = true;
    }
    CHECK(threw);
    CHECK(!a.get() && !b.get() && !c.get() && a.size() == 0 && b.size() == 0 && c.size() == 0);
    CHECK(Fake::live.empty());
    gpu::alloc_group(4, a, b, c);   // and the group is usable again
    CHECK(a.size() == 4 && b.size() == 4 && c.size() == 4 && Fake::live.size() == 3);
  }
  ok("group");
}

void move_case() {
  {
    Buf a;
    a.alloc(7);
    uint32_t* p = a.get();
    const int f = Fake::frees;
    Buf b(std::move(a));   // construction
    CHECK(a.get() == nullptr && a.size() == 0 && b.get() == p && b.size() == 7);
    Buf c;
    c.alloc(9);
    c = std::move(b);      // assignment over a live block: that block is freed, once
    CHECK(b.get() == nullptr && b.size() == 0 && c.get() == p && c.size() == 7);
    CHECK(Fake::frees == f + 1 && Fake::live.size() == 1);
    Buf& self = c;
    c = std::move(self);   // (self-assignment keeps the block)
    CHECK(c.get() == p && c.size() == 7 && Fake::live.size() == 1);
  }
  ok("move");
}

void destruct_case() {
  const int a0 = Fake::allocs, f0 = Fake::frees;
  {
    Buf a, b, empty;
    a.alloc(1);
    b.alloc(2);
    CHECK(Fake::live.size() == 2);
  }
  CHECK(Fake::allocs - a0 == 2 && Fake::frees - f0 == 2);   // each live block once, the empty one none
  ok("destruct");
}

}  // namespace

int main() {
  reserve_case();
  failed_alloc_case();
  group_case();
  move_case();
  destruct_case();
  CHECK(Fake::live.empty());
  return 0;
}
