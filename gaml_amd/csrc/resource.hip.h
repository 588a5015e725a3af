// resource.hip.h -- the GPU resources the library holds, each owned by the object that names it: device and pinned buffers,
// events, streams, a block the host writes, a ring of slots. Every type is move-only and frees in its destructor; an empty
// one makes no runtime call when it goes (host-only contexts never touch the runtime). Whoever destroys them sees to it
// that the device is through with them and that their device is current (gaml_hip_destroy).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <algorithm>
#include <cstddef>
#include <type_traits>
#include <utility>

namespace gaml {
namespace detail {

// grow-only device buffer
struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete; DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p(std::exchange(o.p, nullptr)), cap(std::exchange(o.cap, 0)) {}
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) { reset(); p = std::exchange(o.p, nullptr); cap = std::exchange(o.cap, 0); }
    return *this;
  }
  ~DevBuf() { reset(); }
  void reset() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
  hipError_t reserve(size_t bytes) {
    if (bytes <= cap) return hipSuccess;
    if (p) { hipError_t e = hipFree(p); if (e != hipSuccess) return e; p = nullptr; cap = 0; }
    size_t want = std::max(bytes + bytes / 4, (size_t)256);
    hipError_t e = hipMalloc(&p, want);
    if (e == hipSuccess) cap = want;
    return e;
  }
  // ... for a buffer that launches on `st` may still read: the stream drains before the old one goes
  hipError_t reserve(size_t bytes, hipStream_t st) {
    if (bytes <= cap) return hipSuccess;
    if (p) { hipError_t e = hipStreamSynchronize(st); if (e != hipSuccess) return e; }
    return reserve(bytes);
  }
  // a new allocation of exactly `bytes` that starts with the old one's first `keep` bytes (the caller has made sure that
  // nothing reads the old one any more); on failure the old one stays
  hipError_t regrow(size_t bytes, size_t keep) {
    DevBuf nb;
    hipError_t e = hipMalloc(&nb.p, bytes);
    if (e != hipSuccess) return e;
    nb.cap = bytes;
    if (p && keep) { e = hipMemcpy(nb.p, p, keep, hipMemcpyDeviceToDevice); if (e != hipSuccess) return e; }
    if (p) { e = hipFree(p); if (e != hipSuccess) return e; p = nullptr; cap = 0; }
    *this = std::move(nb);
    return hipSuccess;
  }
  template <class T> T* as() const { return (T*)p; }
};

// grow-only pinned host buffer
struct PinBuf {
  void* p = nullptr;
  void* dev = nullptr;  // the same memory as the device sees it
  size_t cap = 0;
  PinBuf() = default;
  PinBuf(const PinBuf&) = delete; PinBuf& operator=(const PinBuf&) = delete;
  PinBuf(PinBuf&& o) noexcept : p(std::exchange(o.p, nullptr)), dev(std::exchange(o.dev, nullptr)), cap(std::exchange(o.cap, 0)) {}
  PinBuf& operator=(PinBuf&& o) noexcept {
    if (this != &o) { reset(); p = std::exchange(o.p, nullptr); dev = std::exchange(o.dev, nullptr); cap = std::exchange(o.cap, 0); }
    return *this;
  }
  ~PinBuf() { reset(); }
  void reset() { if (p) (void)hipHostFree(p); p = nullptr; dev = nullptr; cap = 0; }
  hipError_t reserve(size_t bytes) {
    if (bytes <= cap) return hipSuccess;
    reset();
    size_t want = std::max(bytes + bytes / 4, (size_t)4096);
    // device-visible (kernels read / write it directly) and coherent: the host polls words the device writes (per-block
    // partials, sequence words) without any runtime call in between
    hipError_t e = hipHostMalloc(&p, want, hipHostMallocMapped | hipHostMallocCoherent);
    if (e == hipSuccess) e = hipHostGetDevicePointer(&dev, p, 0);
    if (e == hipSuccess) cap = want;
    return e;
  }
};

// an event / a stream, made where it is first needed (the handle is public for the runtime's create calls: into an empty one only)
struct Event {
  hipEvent_t e = nullptr;
  Event() = default;
  Event(const Event&) = delete; Event& operator=(const Event&) = delete;
  Event(Event&& o) noexcept : e(std::exchange(o.e, nullptr)) {}
  Event& operator=(Event&& o) noexcept { if (this != &o) { reset(); e = std::exchange(o.e, nullptr); } return *this; }
  ~Event() { reset(); }
  void reset() { if (e) (void)hipEventDestroy(e); e = nullptr; }
  hipError_t ensure(unsigned flags = hipEventDisableTiming) { return e ? hipSuccess : hipEventCreateWithFlags(&e, flags); }
  operator hipEvent_t() const { return e; }
};
struct Stream {
  hipStream_t s = nullptr;
  Stream() = default;
  Stream(const Stream&) = delete; Stream& operator=(const Stream&) = delete;
  Stream(Stream&& o) noexcept : s(std::exchange(o.s, nullptr)) {}
  Stream& operator=(Stream&& o) noexcept { if (this != &o) { reset(); s = std::exchange(o.s, nullptr); } return *this; }
  ~Stream() { reset(); }
  void reset() { if (s) (void)hipStreamDestroy(s); s = nullptr; }
  operator hipStream_t() const { return s; }
};

// A block of device memory that the host writes: fine-grained device memory behind the PCIe BAR (`direct`: plain stores, no
// copy), or ordinary device memory filled from the pinned twin `host`. How large it is and when the twin is reserved is the
// site's business.
struct HostBlock {
  void* dev = nullptr;
  size_t cap = 0;
  bool direct = false;
  PinBuf host;
  HostBlock() = default;
  HostBlock(const HostBlock&) = delete; HostBlock& operator=(const HostBlock&) = delete;
  HostBlock(HostBlock&& o) noexcept : dev(std::exchange(o.dev, nullptr)), cap(std::exchange(o.cap, 0)), direct(o.direct), host(std::move(o.host)) {}
  HostBlock& operator=(HostBlock&& o) noexcept {
    if (this != &o) { reset(); dev = std::exchange(o.dev, nullptr); cap = std::exchange(o.cap, 0); direct = o.direct; host = std::move(o.host); }
    return *this;
  }
  ~HostBlock() { reset(); }
  void reset() { if (dev) (void)hipFree(dev); dev = nullptr; cap = 0; host.reset(); }
  // a new device block of `bytes` (the old one goes first)
  hipError_t alloc(size_t bytes, bool direct_write) {
    if (dev) { hipError_t e = hipFree(dev); if (e != hipSuccess) return e; dev = nullptr; cap = 0; }
    hipError_t e = direct_write ? hipExtMallocWithFlags(&dev, bytes, hipDeviceMallocFinegrained) : hipMalloc(&dev, bytes);
    if (e == hipSuccess) { cap = bytes; direct = direct_write; }
    return e;
  }
  // ... once `st`, whose launches may still read the old one, has drained
  hipError_t reserve(size_t bytes, bool direct_write, hipStream_t st) {
    hipError_t e = hipStreamSynchronize(st);
    return e != hipSuccess ? e : alloc(bytes, direct_write);
  }
};

constexpr int kRing = 4;  // slots, so that async callers may run ahead of the device

// A ring of slots, each with an event that tells when the device is through with it.
template <class Slot>
struct Ring {
  Slot slot[kRing];
  Event done[kRing];
  bool armed[kRing] = {};
  int next = 0;
  // the next slot, once the device is done with what it last held
  hipError_t acquire(int* k_out) {
    const int k = next;
    next = (next + 1) % kRing;
    if (armed[k]) { hipError_t e = hipEventSynchronize(done[k]); if (e != hipSuccess) return e; armed[k] = false; }
    *k_out = k;
    return done[k].ensure();
  }
  // slot k is in use by what `st` holds so far
  hipError_t release(int k, hipStream_t st) {
    hipError_t e = hipEventRecord(done[k], st);
    if (e == hipSuccess) armed[k] = true;
    return e;
  }
};
using Staging = Ring<PinBuf>;   // pinned slots: host data on its way to the device
using Arena = Ring<HostBlock>;  // per-call tables of a paired set (paired_launch.hip.h)

template <class T> constexpr bool owns_v = !std::is_copy_constructible<T>::value && !std::is_copy_assignable<T>::value && std::is_nothrow_move_constructible<T>::value && std::is_nothrow_move_assignable<T>::value;
static_assert(owns_v<DevBuf> && owns_v<PinBuf> && owns_v<Event> && owns_v<Stream> && owns_v<HostBlock> && owns_v<Staging> && owns_v<Arena>,
              "resources are move-only, and moving them cannot fail");

}  // namespace detail
}  // namespace gaml
