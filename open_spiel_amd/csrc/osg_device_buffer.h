// Owners of device and pinned host memory: an allocation goes with the object (or scope) that holds its owner, so a
// handle type keeps no list of what to free and a failure path frees nothing by hand.  These are the only places
// that call the runtime's allocation functions.
#ifndef OSG_DEVICE_BUFFER_H_
#define OSG_DEVICE_BUFFER_H_

#include <hip/hip_runtime.h>

#include <cstddef>
#include <utility>

namespace osg {

// A typed device allocation.  Move-only; reads as its raw pointer where a kernel argument, a view struct or a copy
// wants one, and as null while nothing is allocated.
template <class T>
class DeviceArray {
 public:
  DeviceArray() = default;
  DeviceArray(const DeviceArray&) = delete;
  DeviceArray& operator=(const DeviceArray&) = delete;
  DeviceArray(DeviceArray&& o) noexcept : p_(std::exchange(o.p_, nullptr)), n_(std::exchange(o.n_, 0)) {}
  DeviceArray& operator=(DeviceArray&& o) noexcept {
    if (this != &o) { reset(); p_ = std::exchange(o.p_, nullptr); n_ = std::exchange(o.n_, 0); }
    return *this;
  }
  ~DeviceArray() { reset(); }

  T* get() const { return p_; }
  operator T*() const { return p_; }
  size_t size() const { return n_; }   // capacity in elements (0: nothing allocated)
  void reset() {
    if (p_) (void)hipFree(p_);
    p_ = nullptr; n_ = 0;
  }
  // n elements, uninitialised (n == 0: one element, so that a made buffer is never null).  Frees what was held.
  hipError_t alloc(size_t n) { return take(n, false); }
  // The same in fine-grained memory: peers' stores and system-scope loads meet in memory, not in a cache.
  hipError_t alloc_finegrained(size_t n) { return take(n, true); }
  // Grow-only: reallocates (contents lost) only when n exceeds the capacity; after a failure nothing is held.
  hipError_t ensure(size_t n) { return n <= n_ ? hipSuccess : alloc(n); }

 private:
  hipError_t take(size_t n, bool finegrained) {
    reset();
    if (n == 0) n = 1;
    void* p = nullptr;
    const hipError_t e = finegrained ? hipExtMallocWithFlags(&p, n * sizeof(T), hipDeviceMallocFinegrained) : hipMalloc(&p, n * sizeof(T));
    if (e == hipSuccess) { p_ = static_cast<T*>(p); n_ = n; }
    return e;
  }
  T* p_ = nullptr;
  size_t n_ = 0;
};

// A few words of pinned host memory mapped into the device's address space (a kernel raises or fills them, the host
// reads them without a copy).
template <class T>
class PinnedArray {
 public:
  PinnedArray() = default;
  PinnedArray(const PinnedArray&) = delete;
  PinnedArray& operator=(const PinnedArray&) = delete;
  ~PinnedArray() { reset(); }

  T* get() const { return p_; }
  operator T*() const { return p_; }
  void reset() {
    if (p_) (void)hipHostFree(p_);
    p_ = nullptr;
  }
  hipError_t alloc(size_t n) {
    reset();
    void* p = nullptr;
    const hipError_t e = hipHostMalloc(&p, (n ? n : 1) * sizeof(T), hipHostMallocMapped);
    if (e == hipSuccess) p_ = static_cast<T*>(p);
    return e;
  }

 private:
  T* p_ = nullptr;
};

}  // namespace osg

#endif  // OSG_DEVICE_BUFFER_H_
