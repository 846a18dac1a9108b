// dev_array.hpp -- the one owner of a device array in the host layer (ceed_impl.hpp and the ceed_*.cpp sources).
//
// Every device array a library object owns is a DevArray member: allocated (or uploaded) under the object's Ceed, and gone with
// the member.  There is ONE way out, release(): ceed_retire.  With no hipGraph of the Ceed alive or being recorded that is "drain
// the Ceed's stream, hipFree"; under a graph the array is parked until the last graph goes, so a recorded kernel
// node never points at freed memory -- by construction, not by remembering to route a pointer somewhere.  An array bound to no
// Ceed (a function's scratch; what a Ceed itself owns that no graph outlives) is freed directly.
//
// An empty array still has a valid address: max(n, 1) elements are allocated.  No resizing policy, no host mirror.
// Plain C++ over hip_runtime_api.h: nothing here needs hipcc (tests/dev_array_host.cpp builds it with g++ under sanitizers).
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <vector>

typedef struct Ceed_private *Ceed;   // as include/ceed.h
int ceed_error(const char *fmt, ...);
// park a device allocation that recorded graph nodes may still read; freed with the last graph (or at once, behind the stream, if none)
void ceed_retire(Ceed c, void *p);

template <class T>
struct DevArray {
  DevArray() = default;
  DevArray(const DevArray &) = delete;
  DevArray &operator=(const DevArray &) = delete;
  DevArray(DevArray &&o) noexcept : p(o.p), n(o.n), ceed(o.ceed) { o.p = nullptr; o.n = 0; }
  DevArray &operator=(DevArray &&o) noexcept {
    if (this != &o) { release(); p = o.p; n = o.n; ceed = o.ceed; o.p = nullptr; o.n = 0; }
    return *this;
  }
  ~DevArray() { release(); }

  // `count` elements (uninitialised) under Ceed `c` (null: bound to none); whatever the array held is released first
  int alloc(Ceed c, size_t count) {
    release();
    void *q = nullptr;
    const hipError_t e = hipMalloc(&q, sizeof(T) * (count ? count : 1));
    if (e != hipSuccess) return ceed_error("device allocation of %zu x %zu bytes failed (HIP error %d)", count, sizeof(T), (int)e);
    p = (T *)q; n = count; ceed = c;
    return 0;
  }
  // the same, filled from host memory (a blocking copy); on failure nothing stays allocated
  int upload(Ceed c, const T *src, size_t count) {
    const int ierr = alloc(c, count);
    if (ierr) return ierr;
    const hipError_t e = count ? hipMemcpy(p, src, sizeof(T) * count, hipMemcpyHostToDevice) : hipSuccess;
    if (e == hipSuccess) return 0;
    (void)hipFree(p);   // (no launch has seen it)
    p = nullptr; n = 0;
    return ceed_error("upload of %zu x %zu bytes to the device failed (HIP error %d)", count, sizeof(T), (int)e);
  }
  int upload(Ceed c, const std::vector<T> &v) { return upload(c, v.data(), v.size()); }
  void release() {
    if (!p) return;
    if (ceed) ceed_retire(ceed, p); else (void)hipFree(p);
    p = nullptr; n = 0;
  }
  T *get() const { return p; }
  size_t size() const { return n; }
  explicit operator bool() const { return p != nullptr; }

 private:
  T *p = nullptr;
  size_t n = 0;
  Ceed ceed = nullptr;
};
