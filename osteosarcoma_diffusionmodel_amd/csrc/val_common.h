// val_common.h -- what the validator's translation units (validate.hip, corr.hip, glm.hip and the later ones) share: the
// scope-lifetime device buffer, the wavefront butterflies, the "one wavefront per row" indices, the checked kernel launch, the
// read-back, the column-list upload, the check of a CSR set list and the packer of host tables into one allocation.  What the
// sort-based statistics share on top of this is in val_columns.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <vector>
#include "handle.h"

namespace osd {

// A device allocation of bytes, freed on scope exit (devmem.h).  A request for 0 bytes allocates 16: never null after a successful alloc.
struct ValBuf : DevBuf<char> {
  int alloc(size_t bytes) { return reserve((int64_t)(bytes ? bytes : 16)); }
  template <class T> T* as() const { return reinterpret_cast<T*>(get()); }
};

// Butterflies over the 64 lanes, in place, xor distances 32, 16, ... 1: every lane ends with the result, and the fixed order gives
// the same bits on every call.  Several values (float, double, int, long long, unsigned long long, mixed) share one walk, so their
// exchanges overlap.
template <class T> __device__ __forceinline__ void lane_max(T& v, int o) { const T x = __shfl_xor(v, o); v = x > v ? x : v; }
template <class T> __device__ __forceinline__ void lane_min(T& v, int o) { const T x = __shfl_xor(v, o); v = x < v ? x : v; }
template <class... T> __device__ __forceinline__ void wave_sum(T&... v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) ((v += __shfl_xor(v, o)), ...);
}
template <class... T> __device__ __forceinline__ void wave_max(T&... v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) (lane_max(v, o), ...);
}
template <class... T> __device__ __forceinline__ void wave_min(T&... v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) (lane_min(v, o), ...);
}

// One wavefront per row over a 1-D grid: the lane, the wavefront's number in the grid (its first row) and the number of wavefronts
// (its stride).  I: the type the row index is computed in.  Call it as wave_rows(): the default arguments are evaluated in the
// calling kernel, where the compiler knows that workgroups are uniform and reads blockDim straight from the kernel arguments.
template <class I> struct WaveRows { int lane; I wave, nw; };
template <class I = int64_t>
__device__ __forceinline__ WaveRows<I> wave_rows(unsigned tid = threadIdx.x, unsigned bid = blockIdx.x, unsigned bdim = blockDim.x,
                                                 unsigned gdim = gridDim.x) {
  return {(int)(tid & 63), (I)((bid * (I)bdim + tid) >> 6), (I)(((I)gdim * bdim) >> 6)};
}

// A kernel launch and its launch-error check: OSD_HIP(launched(kernel, grid, block, lds_bytes, stream, args...)).
template <class... P, class... A>
inline hipError_t launched(void (*kernel)(P...), dim3 grid, dim3 block, size_t lds_bytes, hipStream_t s, A... args) {
  hipLaunchKernelGGL(kernel, grid, block, lds_bytes, s, args...);
  return hipGetLastError();
}

// dev -> host on the stream, then wait for the stream: the end of a synchronous entry point that returns host values
inline hipError_t read_back(hipStream_t s, void* host, const void* dev, size_t bytes) {
  const hipError_t e = hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, s);
  return e != hipSuccess ? e : hipStreamSynchronize(s);
}

// A host column list, checked (1 <= g <= limit indices in [0, ld)) before anything touches the device; then the device is
// selected and the list uploaded into dc on the stream.
inline int upload_cols(int device, hipStream_t s, const int32_t* cols_host, int g, int ld, int limit, ValBuf& dc) {
  if (!cols_host || g < 1 || g > limit) { set_error("bad column list (1 <= columns <= %d)", limit); return OSD_EINVAL; }
  for (int i = 0; i < g; ++i)
    if (cols_host[i] < 0 || cols_host[i] >= ld) { set_error("column index out of range"); return OSD_EINVAL; }
  OSD_HIP(hipSetDevice(device));
  OSD_TRY(dc.alloc((size_t)g * sizeof(int)));
  OSD_HIP(hipMemcpyAsync(dc.get(), cols_host, (size_t)g * sizeof(int), hipMemcpyHostToDevice, s));
  return OSD_OK;
}

// A host list of S sets in CSR form over [0, D), checked before anything touches the device: offsets start at 0, every set has
// 1 <= members <= max_members and fewer than D, every member lies in [0, D) and occurs once in its set.  The error texts call a
// member a `noun` ("position", "column") and a set's size `size` ('k', 'm').  seen [D]: the last set that holds each index, or -1.
inline int check_sets(const int32_t* offsets, const int32_t* members, int S, int D, int max_members, const char* noun, char size,
                      std::vector<int32_t>& seen) {
  if (offsets[0] != 0) { set_error("set_offsets must start at 0"); return OSD_EINVAL; }
  seen.assign((size_t)D, -1);
  for (int s = 0; s < S; ++s) {
    const int64_t k = (int64_t)offsets[s + 1] - offsets[s];
    if (k < 1 || k > max_members || k >= D) {
      set_error("set %d has %lld members: 1 <= %c <= %d and %c < D are needed", s, (long long)k, size, max_members, size);
      return OSD_EINVAL;
    }
    for (int32_t e = offsets[s]; e < offsets[s + 1]; ++e) {
      const int32_t g = members[e];
      if (g < 0 || g >= D) { set_error("set %d holds the %s %d outside [0, %d)", s, noun, g, D); return OSD_EINVAL; }
      if (seen[g] == s) { set_error("set %d holds the %s %d more than once", s, noun, g); return OSD_EINVAL; }
      seen[g] = s;
    }
  }
  return OSD_OK;
}

// One device allocation carved at multiples of 256 bytes.  put() reserves room for a host table and stages it, take() reserves room
// the device fills; after alloc(), upload() sends every staged table in one copy (put the tables first: the copy ends at the last
// one).  The staging vector lives as long as the packer, and the caller waits for the stream before it relies on that no longer.
struct Packed {
  size_t bytes = 0;
  std::vector<char> host;
  ValBuf ws;
  size_t take(size_t n) { const size_t at = bytes; bytes += (n + 255) & ~(size_t)255; return at; }
  size_t put(const void* table, size_t n) {
    const size_t at = take(n);
    host.resize(bytes);
    if (n) memcpy(host.data() + at, table, n);
    return at;
  }
  int alloc() { return ws.alloc(bytes); }
  hipError_t upload(hipStream_t s) { return hipMemcpyAsync(ws.get(), host.data(), host.size(), hipMemcpyHostToDevice, s); }
  template <class T> T* at(size_t offset) const { return reinterpret_cast<T*>(ws.get() + offset); }
};

}  // namespace osd
