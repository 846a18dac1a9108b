// dev_array_host.cpp -- DevArray (ceedpetscsolid_amd/csrc/dev_array.hpp) on the host alone, built with g++ under the address and
// undefined-behaviour sanitizers by test_dev_array_host.py.  No HIP runtime is linked: hipMalloc / hipFree / hipMemcpy are
// malloc-backed stand-ins that keep a ledger of what is allocated (hipMalloc can be told to fail at its k-th call), ceed_retire
// parks into a list while a "graph live" flag is set, exactly as the library's does, and ceed_error records and returns.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <utility>
#include <vector>

#include "dev_array.hpp"

// ---------------------------------------------------------------------------
// the stand-ins
// ---------------------------------------------------------------------------
static std::set<void *> g_live;          // allocated and not yet freed
static int g_mallocs = 0, g_fail_at = 0; // calls of hipMalloc so far; the call that fails (0: none)
static int g_errors = 0;
static int g_failures = 0;

struct Ceed_private { bool graph_live = false; std::vector<void *> parked; int drains = 0; };

extern "C" hipError_t hipMalloc(void **ptr, size_t size) {
  if (++g_mallocs == g_fail_at) { *ptr = nullptr; return hipErrorOutOfMemory; }
  if (size == 0) { *ptr = nullptr; return hipSuccess; }     // as the runtime: DevArray must never ask for this
  *ptr = malloc(size);
  g_live.insert(*ptr);
  return hipSuccess;
}
extern "C" hipError_t hipFree(void *ptr) {
  if (!ptr) return hipSuccess;
  if (!g_live.erase(ptr)) { fprintf(stderr, "FAIL: hipFree of %p, which is not allocated\n", ptr); g_failures++; return hipErrorInvalidValue; }
  free(ptr);
  return hipSuccess;
}
extern "C" hipError_t hipMemcpy(void *dst, const void *src, size_t size, hipMemcpyKind) {
  memcpy(dst, src, size);
  return hipSuccess;
}
int ceed_error(const char *fmt, ...) {
  char msg[256];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(msg, sizeof msg, fmt, ap);
  va_end(ap);
  g_errors++;
  return 1;
}
void ceed_retire(Ceed c, void *p) {
  if (!p) return;
  if (c->graph_live) c->parked.push_back(p);
  else { c->drains++; (void)hipFree(p); }
}
static void free_parked(Ceed c) {
  for (void *p : c->parked) (void)hipFree(p);
  c->parked.clear();
}

#define EXPECT(cond) do { if (!(cond)) { fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); g_failures++; } } while (0)

// ---------------------------------------------------------------------------
// the cases
// ---------------------------------------------------------------------------
static void sizes(Ceed c) {
  for (size_t n : {(size_t)0, (size_t)1, (size_t)1000}) {
    for (Ceed bound : {c, (Ceed) nullptr}) {
      DevArray<double> a;
      EXPECT(!a && a.get() == nullptr && a.size() == 0);
      EXPECT(a.alloc(bound, n) == 0);
      EXPECT(a && a.get() != nullptr && a.size() == n);      // an empty array has an address too
      EXPECT(g_live.size() == 1);
      if (n) a.get()[n - 1] = 1.;                            // (the sanitizer sees a short allocation)
      a.release();
      EXPECT(!a && a.size() == 0 && g_live.empty());
      a.release();                                           // a second release is nothing

      std::vector<uint32_t> h(n);
      for (size_t i = 0; i < n; i++) h[i] = (uint32_t)(3 * i + 1);
      DevArray<uint32_t> u;
      EXPECT(u.upload(bound, h) == 0);
      EXPECT(u && u.size() == n && g_live.size() == 1);
      EXPECT(n == 0 || memcmp(u.get(), h.data(), n * sizeof(uint32_t)) == 0);
      DevArray<uint32_t> v;
      EXPECT(v.upload(bound, h.data(), n) == 0);
      EXPECT(g_live.size() == 2);
    }                                                        // the destructors release
    EXPECT(g_live.empty());
  }
}
static void moves(Ceed c) {
  DevArray<int> a;
  EXPECT(a.alloc(c, 7) == 0);
  int *pa = a.get();
  DevArray<int> b(std::move(a));
  EXPECT(!a && a.size() == 0 && b.get() == pa && b.size() == 7 && g_live.size() == 1);
  a.release();                                               // a moved-from array releases nothing
  EXPECT(g_live.size() == 1);
  DevArray<int> d;
  EXPECT(d.alloc(c, 3) == 0);
  EXPECT(g_live.size() == 2);
  d = std::move(b);                                          // what d held goes, b's array has one owner: d
  EXPECT(!b && d.get() == pa && d.size() == 7 && g_live.size() == 1 && g_live.count(pa));
  { DevArray<int> gone(std::move(a)); }                      // moved-from twice over: nothing to free
  EXPECT(g_live.size() == 1);
  std::vector<DevArray<int>> vec;                            // as a container element (an operator's lists)
  vec.push_back(std::move(d));
  vec.emplace_back();
  EXPECT(vec.back().alloc(c, 2) == 0);
  vec.emplace_back(); vec.emplace_back(); vec.emplace_back();  // reallocation moves the elements
  EXPECT(g_live.size() == 2 && vec[0].get() == pa);
  vec.clear();
  EXPECT(g_live.empty());
}
static void second_upload(Ceed c) {
  const std::vector<double> one(10, 1.), two(20, 2.);
  DevArray<double> a;
  EXPECT(a.upload(c, one) == 0);
  EXPECT(a.upload(c, two) == 0);                             // the first array is released, not leaked
  EXPECT(g_live.size() == 1 && a.size() == 20 && a.get()[19] == 2.);
  EXPECT(a.alloc(c, 5) == 0);
  EXPECT(g_live.size() == 1 && a.size() == 5);
}
static void parking(Ceed c) {
  void *p0 = nullptr, *p1 = nullptr;
  c->graph_live = true;
  {
    DevArray<double> a, b;
    EXPECT(a.alloc(c, 100) == 0 && b.alloc(c, 100) == 0);
    p0 = a.get(); p1 = b.get();
    a.release();                                             // parked, not freed: a recorded launch may still read it
    EXPECT(c->parked.size() == 1 && c->parked[0] == p0 && g_live.count(p0) == 1);
    EXPECT(a.alloc(c, 200) == 0);                            // (and the array is usable again at once)
    DevArray<double> unbound;
    EXPECT(unbound.alloc(nullptr, 4) == 0);                  // bound to no Ceed: freed directly whatever the flag says
    void *pu = unbound.get();
    unbound.release();
    EXPECT(g_live.count(pu) == 0 && c->parked.size() == 1);
  }                                                          // b and the second a leave through the same exit
  EXPECT(c->parked.size() == 3 && g_live.size() == 3 && g_live.count(p0) && g_live.count(p1));
  c->graph_live = false;
  free_parked(c);
  EXPECT(g_live.empty());
}
// an object of three arrays uploaded in turn, as the library's Create functions do; its destructor is the clean-up
struct Three {
  DevArray<uint32_t> rowptr, cols;
  DevArray<double> vals;
  int build(Ceed c) {
    const std::vector<uint32_t> rp{0, 1, 3}, cl{0, 0, 1};
    const std::vector<double> v{1., 2., 3.};
    int ierr;
    if ((ierr = rowptr.upload(c, rp))) return ierr;
    if ((ierr = cols.upload(c, cl))) return ierr;
    if ((ierr = vals.upload(c, v))) return ierr;
    return 0;
  }
};
static void failing_malloc(Ceed c) {
  for (int k = 1; k <= 4; k++) {
    const int errors_before = g_errors;
    g_mallocs = 0; g_fail_at = k;
    {
      Three t;
      const int ierr = t.build(c);
      if (k <= 3) {
        EXPECT(ierr != 0 && g_errors == errors_before + 1);
        EXPECT((int)g_live.size() == k - 1);                 // what was built before the failure, still owned
        EXPECT(bool(t.rowptr) == (k > 1) && bool(t.cols) == (k > 2) && !t.vals);
      } else {
        EXPECT(ierr == 0 && g_live.size() == 3 && t.vals.get()[2] == 3.);
      }
    }
    EXPECT(g_live.empty());                                  // nothing leaks, whichever allocation failed
  }
  g_fail_at = 0;
  // a failing re-allocation leaves the array empty, not dangling
  DevArray<int> a;
  EXPECT(a.alloc(c, 8) == 0);
  g_mallocs = 0; g_fail_at = 1;
  EXPECT(a.alloc(c, 16) != 0);
  g_fail_at = 0;
  EXPECT(!a && a.size() == 0 && g_live.empty());
}

int main() {
  Ceed_private ceed;
  sizes(&ceed);
  moves(&ceed);
  second_upload(&ceed);
  parking(&ceed);
  failing_malloc(&ceed);
  EXPECT(g_live.empty() && ceed.parked.empty());
  EXPECT(ceed.drains > 0);                                   // the bound arrays did leave through ceed_retire
  if (g_failures) { fprintf(stderr, "%d check(s) failed\n", g_failures); return 1; }
  printf("dev_array_host ok\n");
  return 0;
}
