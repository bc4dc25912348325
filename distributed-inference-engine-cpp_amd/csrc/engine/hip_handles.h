// Move-only owners of the HIP objects the engine holds: device memory, pinned host memory, streams,
// events and instantiated graphs.  A handle releases its object when it is destroyed, so whatever a
// constructor had made before it threw goes back to the device.  The create calls return the HIP
// status (wrap them in HIP_CHECK); the implicit conversion keeps the call sites of the raw type.
#pragma once

#include <hip/hip_runtime.h>

namespace die {
namespace hip {

template <class T, class Raw, hipError_t (*Release)(Raw)>
class Handle {
 public:
  Handle() = default;
  Handle(Handle&& o) noexcept : h_(o.h_) { o.h_ = T{}; }
  Handle& operator=(Handle&& o) noexcept {
    if (this != &o) {
      reset();
      h_ = o.h_;
      o.h_ = T{};
    }
    return *this;
  }
  ~Handle() { reset(); }
  T get() const { return h_; }
  operator T() const { return h_; }
  void reset() {
    if (h_) (void)Release(h_);
    h_ = T{};
  }

 protected:
  T h_{};
};

template <class T>
struct DeviceMem : Handle<T*, void*, hipFree> {
  hipError_t alloc(size_t bytes) {
    this->reset();
    return hipMalloc(reinterpret_cast<void**>(&this->h_), bytes);
  }
};

template <class T>
struct PinnedMem : Handle<T*, void*, hipHostFree> {
  hipError_t alloc(size_t bytes, unsigned flags = hipHostMallocDefault) {
    this->reset();
    return hipHostMalloc(reinterpret_cast<void**>(&this->h_), bytes, flags);
  }
};

struct Stream : Handle<hipStream_t, hipStream_t, hipStreamDestroy> {
  hipError_t create(unsigned flags = hipStreamNonBlocking) {
    reset();
    return hipStreamCreateWithFlags(&h_, flags);
  }
};

struct Event : Handle<hipEvent_t, hipEvent_t, hipEventDestroy> {
  hipError_t create(unsigned flags = hipEventDefault) {
    reset();
    return hipEventCreateWithFlags(&h_, flags);
  }
};

struct GraphExec : Handle<hipGraphExec_t, hipGraphExec_t, hipGraphExecDestroy> {
  hipError_t instantiate(hipGraph_t g) {
    reset();
    return hipGraphInstantiate(&h_, g, nullptr, nullptr, 0);
  }
};

}  // namespace hip
}  // namespace die
