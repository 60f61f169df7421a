// devmem.h -- the owning types behind osd_handle and its satellites.  Whatever a handle allocates on the device, stages on the host or
// creates in the runtime is a member of one of these, so deleting the handle releases it and no release list is kept by hand.
// Host code only.  Included by handle.h, behind OSD_HIP / OSD_TRY / device_alloc.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <algorithm>
#include <utility>
#include <vector>

namespace osd {

// A runtime object destroyed with its owner; null until put() hands its address to the runtime's create call.  Move-only.
template <class H, hipError_t (*Destroy)(H)>
class Owned {
 public:
  Owned() = default;
  Owned(Owned&& o) noexcept : h_(o.h_) { o.h_ = nullptr; }
  Owned& operator=(Owned&& o) noexcept { std::swap(h_, o.h_); return *this; }
  ~Owned() { reset(); }
  operator H() const { return h_; }
  void reset(H h = nullptr) {
    if (h_) { hipError_t e = Destroy(h_); (void)e; }
    h_ = h;
  }
  H* put() { reset(); return &h_; }
 private:
  H h_ = nullptr;
};
using Event = Owned<hipEvent_t, hipEventDestroy>;
using Stream = Owned<hipStream_t, hipStreamDestroy>;
using Graph = Owned<hipGraph_t, hipGraphDestroy>;
using GraphExec = Owned<hipGraphExec_t, hipGraphExecDestroy>;

// A grow-only device buffer of T, freed with its owner; reads as the T* it holds.  Move-only.  reserve(n) makes room for n elements:
// nothing happens while the capacity suffices, else the old allocation is freed (its contents are not kept) and a new one of exactly
// n elements made through device_alloc -- so every out-of-memory reads OSD_ENOMEM with the byte count.  reserve(n, stream) waits for
// that stream before it frees an old allocation that work queued there may still use; any stream is one, the null stream included.
template <class T>
class DevBuf {
 public:
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr; o.cap_ = 0; }
  DevBuf& operator=(DevBuf&& o) noexcept { std::swap(p_, o.p_); std::swap(cap_, o.cap_); return *this; }
  ~DevBuf() { if (p_) { hipError_t e = hipFree(p_); (void)e; } }
  int reserve(int64_t n) { return grow(n, nullptr); }
  int reserve(int64_t n, hipStream_t drain) { return grow(n, &drain); }
  operator T*() const { return p_; }
  T* get() const { return p_; }
  int64_t cap() const { return cap_; }      // elements
 private:
  int grow(int64_t n, const hipStream_t* drain) {
    if (cap_ >= n) return OSD_OK;
    if (p_) {
      if (drain) OSD_HIP(hipStreamSynchronize(*drain));
      OSD_HIP(hipFree(p_));
      p_ = nullptr; cap_ = 0;
    }
    OSD_TRY(device_alloc(reinterpret_cast<void**>(&p_), (size_t)n * sizeof(T)));
    cap_ = n;
    return OSD_OK;
  }
  T* p_ = nullptr;
  int64_t cap_ = 0;
};

// A table that calls rewrite on the host and upload: the host staging, the device table and the event that says the last upload has
// read the staging, all made on first use with the size the first call asks for.  A call takes staging() -- which waits for that
// event, so the previous call's copy is never overwritten under it --, fills what it needs and send()s ranges of it; each send
// records the event again.  Neither waits for the device to have used the table: the streams' order does that.
template <class T>
class Staged {
 public:
  Staged() = default;
  ~Staged() { free(host_); }
  // both sides of n elements without the wait: for a caller that may find nothing to upload (api.hip: upload_null_cond)
  int ensure(size_t n) {
    if (!host_) {
      host_ = static_cast<T*>(malloc(n * sizeof(T)));
      if (!host_) { set_error("out of host memory"); return OSD_ENOMEM; }
    }
    if (!ev_) OSD_HIP(hipEventCreateWithFlags(ev_.put(), hipEventDisableTiming));
    return dev_.reserve((int64_t)n);
  }
  int staging(size_t n, T** host) {
    OSD_TRY(ensure(n));
    OSD_HIP(hipEventSynchronize(ev_));
    *host = host_;
    return OSD_OK;
  }
  // elements [off, off + n) of the staging to the same elements of the device table, on s
  int send(size_t off, size_t n, hipStream_t s) {
    OSD_HIP(hipMemcpyAsync(dev_ + off, host_ + off, n * sizeof(T), hipMemcpyHostToDevice, s));
    OSD_HIP(hipEventRecord(ev_, s));
    return OSD_OK;
  }
  T* dev() const { return dev_; }
  const T* host() const { return host_; }
 private:
  T* host_ = nullptr;
  DevBuf<T> dev_;
  Event ev_;
};

// A list the device holds a copy of, uploaded again only when it changed (first step, another batch size, a re-allocated arena): the
// lists hold workspace pointers only, so a DataLoader's fresh tensors every batch cost neither a copy nor a wait.  A changed list
// waits for s first -- the old copy may still be in use.  same(a, b) compares two elements: memcmp where the callers zero every
// element before filling it, field by field where padding bytes would report a change on every step.
template <class E>
struct DevList {
  std::vector<E> kept;
  DevBuf<E> dev;      // at least 64 elements
  template <class Eq>
  int upload(hipStream_t s, const std::vector<E>& fresh, Eq same) {
    if (dev && fresh.size() == kept.size() && std::equal(fresh.begin(), fresh.end(), kept.begin(), same)) return OSD_OK;
    OSD_HIP(hipStreamSynchronize(s));
    OSD_TRY(dev.reserve((int64_t)std::max<size_t>(fresh.size(), 64)));
    kept = fresh;
    if (!kept.empty()) OSD_HIP(hipMemcpyAsync(dev, kept.data(), kept.size() * sizeof(E), hipMemcpyHostToDevice, s));
    return OSD_OK;
  }
};

}  // namespace osd
