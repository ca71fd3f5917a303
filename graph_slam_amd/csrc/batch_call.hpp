// Host-side plumbing shared by the stand-alone fgo_*_batch entry points (two-view BA, plane check, IMU check, VRO RANSAC, descriptor matching, plane
// extraction, plane propagation, map fusion, map cleaning, map normals, map rendering): input validators, device selection, the one device allocation a call
// stages its arrays in, the capped grid and the kernel timer.  An entry point decides every FGO_EINVAL, and n == 0 -> FGO_OK, with the validators alone, before select_device() makes the first HIP call.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <cassert>
#include <cmath>
#include <vector>
#include "../../include/fgo.h"
#include "pose_host.hpp"

namespace fgo {

// a quaternion that can be normalised: its squared norm is positive and finite
inline bool quat_ok(const double *q) {
  const double qq = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3];
  return qq > 0 && std::isfinite(qq);
}
inline bool in_closed(double v, double lo, double hi) { return v >= lo && v <= hi; }      // false for a NaN
// pinhole intrinsics: fx, fy and z_scale positive and finite, cx and cy finite (the depth range is each call's own rule)
inline bool pinhole_ok(double fx, double fy, double cx, double cy, double z_scale) {
  return fx > 0 && fy > 0 && z_scale > 0 && std::isfinite(fx) && std::isfinite(fy) && std::isfinite(z_scale) && std::isfinite(cx) && std::isfinite(cy);
}
// rt (12 x n: pose_rt of every pose, times the extrinsic if there is one), or false if a quaternion cannot be normalised
inline bool poses_rt(const double *pose7, int64_t n, const double *ext7, std::vector<double> &rt) {
  bool ok = !ext7 || quat_ok(ext7 + 3);
  for (int64_t f = 0; f < n && ok; ++f) ok = quat_ok(pose7 + 7 * f + 3);
  rt.resize(ok ? 12 * (size_t)n : 0);
  for (int64_t f = 0; f < n && ok; ++f) pose_rt(pose7 + 7 * f, ext7, rt.data() + 12 * f);
  return ok;
}
// a ptr array (n rows, n + 1 entries) is non-negative and non-decreasing, and no row holds more than max_per_row entries
inline bool csr_ptr_ok(const int64_t *ptr, int64_t n, int64_t max_per_row) {
  if (ptr[0] < 0) return false;
  for (int64_t r = 0; r < n; ++r)
    if (ptr[r + 1] < ptr[r] || ptr[r + 1] - ptr[r] > max_per_row) return false;
  return true;
}

inline int select_device(int device) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return FGO_ENODEV;   // no CPU fallback
  if (hipSetDevice(device) != hipSuccess) return FGO_ENODEV;
  return FGO_OK;
}

// Every device array of a call lives in ONE allocation: a call costs one hipMalloc / hipFree whatever it asks for.  reserve() hands
// out offsets (256-byte aligned) before the allocation is made, at() turns them into pointers afterwards.
struct Arena {
  char *base = nullptr;
  size_t total = 0;
  ~Arena() { if (base) (void)hipFree(base); }
  size_t reserve(size_t bytes) { const size_t o = total; total += (bytes + 255) & ~(size_t)255; return o; }
  hipError_t alloc() { return hipMalloc((void **)&base, total ? total : 1); }
  template <class T> T *at(size_t off) const { return reinterpret_cast<T *>(base + off); }
};

// the workgroups of a launch over `items` items, per_group to a workgroup: at least one and at most grid_cap() -- 2^20 unless
// fgo_debug_grid_cap lowered it (batch_call.cpp) -- the kernels stride beyond that
constexpr unsigned GRID_CAP_DEFAULT = 1u << 20;
unsigned grid_cap();
inline unsigned grid_for(unsigned long long items, unsigned per_group) {
  const unsigned long long g = (items + per_group - 1) / per_group, cap = grid_cap();
  return (unsigned)(g < 1 ? 1 : g > cap ? cap : g);
}

// The kernel time a debug hook reports: a pair of events on the null stream around the launches of a call.  ms() does not wait: it
// comes after something that synchronised behind stop() -- a blocking hipMemcpy or hipDeviceSynchronize -- and is 0.0 when no time can be had.
struct KernelTimer {
  hipEvent_t a = nullptr, b = nullptr;
  ~KernelTimer() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); }
  bool start() {                                 // false: the events could not be created, nothing is recorded
    if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) return false;
    (void)hipEventRecord(a, 0);
    return true;
  }
  void stop() { (void)hipEventRecord(b, 0); }
  double ms() const { float t = 0; return hipEventElapsedTime(&t, a, b) == hipSuccess ? (double)t : 0.0; }
};

// The arrays of a call, staged in one Arena in the order they are named.  in() names an array that upload() copies to the device,
// out() one that download() copies back; both return a handle for ptr().  An array whose host pointer is NULL is absent -- nothing
// is reserved and ptr() gives NULL -- unless out() is told `always`: the device side is then there for the kernel to work in
// (scratch, or an output the kernel needs whether or not the caller wants it) and only the copy back is skipped.
struct Staged {
  static constexpr int CAP = 24;
  struct Entry { const void *src; void *dst; size_t bytes, off; bool present; };
  Arena mem;
  Entry e[CAP];
  int n = 0;

  int in(const void *host, size_t bytes) { return add({host, nullptr, bytes, 0, host != nullptr}); }
  int out(void *host, size_t bytes, bool always = false) { return add({nullptr, host, bytes, 0, host != nullptr || always}); }
  int alloc() { return mem.alloc() == hipSuccess ? FGO_OK : FGO_ENOMEM; }
  int upload() const {
    for (int k = 0; k < n; ++k)
      if (e[k].src && e[k].bytes && hipMemcpy(mem.base + e[k].off, e[k].src, e[k].bytes, hipMemcpyHostToDevice) != hipSuccess) return FGO_ENUM;
    return FGO_OK;
  }
  int download() const {
    for (int k = 0; k < n; ++k)
      if (e[k].dst && e[k].bytes && hipMemcpy(e[k].dst, mem.base + e[k].off, e[k].bytes, hipMemcpyDeviceToHost) != hipSuccess) return FGO_ENUM;
    return FGO_OK;
  }
  template <class T> T *ptr(int h) const { return e[h].present ? mem.at<T>(e[h].off) : nullptr; }

 private:
  int add(Entry x) {
    assert(n < CAP);
    if (x.present) x.off = mem.reserve(x.bytes);
    e[n] = x;
    return n++;
  }
};

}  // namespace fgo
